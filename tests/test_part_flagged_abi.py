"""CPU-side checks of fgi_part_last_flagged (C-ABI 0.4): the header declares it, the library exports it and
the ctypes binding declares its signature and a Graph method for it."""
import ctypes
import os

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "fgi.h")
NAME = "fgi_part_last_flagged"


def test_header_declares_the_entry_point(pkg):
    assert NAME in pkg.fgi.header_symbols(HEADER), f"{NAME} is not declared in include/fgi.h"


def test_library_exports_the_entry_point(pkg):
    assert hasattr(pkg.load_library(), NAME), f"libfgi.so does not export {NAME}"


def test_binding_declares_the_signature(pkg):
    u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    assert pkg.fgi.SIGNATURES[NAME] == [ctypes.c_void_p, u32p, u32p, u32p, ctypes.c_uint64, u64p]
    assert hasattr(pkg.Graph, "part_last_flagged")


def test_version_is_at_least_0_4(pkg):
    lib = pkg.load_library()
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.fgi_version(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) >= (0, 4)
