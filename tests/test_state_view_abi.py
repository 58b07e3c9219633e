"""CPU-side checks of the host-memory state view's boundary (C-ABI 0.6): the header declares the entry
points, the library exports them, the binding declares their signatures, and the plane encoding the GPU
tests compare against (`planes_from_flags`) round-trips every canonical state_flags value."""
import ctypes
import os

import numpy as np

from conftest import ROOT
from test_gpu_state_view import PLANES, flags_from_planes, planes_from_flags

HEADER = os.path.join(ROOT, "include", "fgi.h")
ENTRY_POINTS = ["fgi_state_view_open", "fgi_state_view_close", "fgi_state_view_stats"]
HELPERS = ["fgi_view_flags", "fgi_view_is_consistent"]

# every canonical state_flags value of a registered node (fgi.h): Computing with any of IOSO / DelayStarted,
# Consistent with DelayStarted or not, Invalidated; each with and without hasDelay
CANONICAL = [st | hd for hd in (0, 16) for st in (0, 4, 8, 12, 1, 9, 2)]


def test_header_library_and_binding_agree(pkg):
    txt = open(HEADER).read()
    names = pkg.fgi.header_symbols(HEADER)
    lib = pkg.load_library()
    for n in ENTRY_POINTS + HELPERS:
        assert n in names, f"{n} is not declared in fgi.h"
        assert hasattr(lib, n), f"libfgi.so does not export {n}"
        assert n in pkg.fgi.SIGNATURES, f"the binding declares no signature for {n}"
    assert "typedef struct fgi_state_view" in txt and "typedef struct fgi_view_stats" in txt
    # the binding's struct is the header's: a size word, the handle count, the word count, seven pointers
    assert ctypes.sizeof(pkg.fgi.StateViewStruct) == 16 + 7 * ctypes.sizeof(ctypes.c_void_p)
    assert [f for f, _ in pkg.fgi.StateViewStruct._fields_][3:9] == list(PLANES)
    assert ctypes.sizeof(pkg.fgi.ViewStats) == 32


def test_version_is_0_6(pkg):
    lib = pkg.load_library()
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.fgi_version(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) >= (0, 6)


def test_planes_round_trip_every_canonical_value():
    # 70 handles (a partial second word): every canonical value, empty handles in between and at the end
    flags = np.array((CANONICAL + [0]) * 5, np.uint32)[:70]
    versions = np.where(np.arange(70) % 15 == 14, 0, 1 + np.arange(70)).astype(np.uint64)
    planes = planes_from_flags(versions, flags)
    assert all(len(planes[k]) == 2 and planes[k].dtype == np.uint64 for k in PLANES)
    want = np.where(versions != 0, flags, 0).astype(np.uint32)
    assert set(want.tolist()) == set(CANONICAL) | {0}
    assert np.array_equal(flags_from_planes(planes, 70), want)
    # bits past the last handle stay clear
    assert all(int(planes[k][1]) >> 6 == 0 for k in PLANES)


def test_exported_helpers_decode_like_the_header(pkg):
    """The library's exported copies of the inline helpers (for bindings that cannot inline C) read a view
    built by hand in ordinary memory: they touch no device."""
    lib = pkg.load_library()
    flags = np.array((CANONICAL + [0]) * 5, np.uint32)[:70]
    versions = np.where(np.arange(70) % 15 == 14, 0, 1 + np.arange(70)).astype(np.uint64)
    planes = planes_from_flags(versions, flags)
    sv = pkg.fgi.StateViewStruct()
    sv.struct_size, sv.n_handles, sv.words = ctypes.sizeof(sv), 70, 2
    for k in PLANES:
        setattr(sv, k, planes[k].ctypes.data)
    want = np.where(versions != 0, flags, 0)
    for h in range(72):   # two handles past the end: 0
        exp = int(want[h]) if h < 70 else 0
        assert lib.fgi_view_flags(ctypes.byref(sv), h) == exp, h
        assert lib.fgi_view_is_consistent(ctypes.byref(sv), h) == int(h < 70 and versions[h] != 0 and (exp & 3) == 1), h
