"""CPU-side checks of the sharded partition loads (C-ABI 0.5): the header declares the four entry points, the
library exports them and the ctypes binding declares their signatures and the methods / functions for them."""
import ctypes
import os

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "fgi.h")
NAMES = ["fgi_part_register_shard", "fgi_part_load_edges_shard", "fgi_part_local_register_shards",
         "fgi_part_local_load_shards"]


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_the_entry_point(pkg, name):
    assert name in pkg.fgi.header_symbols(HEADER), f"{name} is not declared in include/fgi.h"


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_the_entry_point(pkg, name):
    assert hasattr(pkg.load_library(), name), f"libfgi.so does not export {name}"


def test_binding_declares_the_signatures(pkg):
    u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    gp = ctypes.POINTER(ctypes.c_void_p)
    sig = pkg.fgi.SIGNATURES
    assert sig["fgi_part_register_shard"] == [ctypes.c_void_p, ctypes.c_uint32, u32p, u64p, u32p]
    assert sig["fgi_part_load_edges_shard"] == [ctypes.c_void_p, ctypes.c_uint64, u32p, u32p, u64p]
    assert sig["fgi_part_local_register_shards"] == [gp, ctypes.c_uint32, u32p, ctypes.POINTER(u32p),
                                                     ctypes.POINTER(u64p), ctypes.POINTER(u32p)]
    assert sig["fgi_part_local_load_shards"] == [gp, ctypes.c_uint32, u64p, ctypes.POINTER(u32p), ctypes.POINTER(u32p),
                                                 ctypes.POINTER(u64p)]
    assert hasattr(pkg.Graph, "part_register_shard") and hasattr(pkg.Graph, "part_load_edges_shard")
    assert callable(pkg.fgi.part_local_register_shards) and callable(pkg.fgi.part_local_load_shards)


def test_version_is_at_least_0_5(pkg):
    lib = pkg.load_library()
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.fgi_version(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) >= (0, 5)
