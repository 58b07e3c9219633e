"""CPU-side checks of the flagged-set entry points (fgi_last_wave_flagged, fgi_wave_wait_flagged): the
header declares them, the library exports them and the ctypes binding declares their signatures."""
import ctypes
import os

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "fgi.h")
NAMES = ("fgi_last_wave_flagged", "fgi_wave_wait_flagged")


def test_header_declares_flagged_entry_points(pkg):
    names = pkg.fgi.header_symbols(HEADER)
    for n in NAMES:
        assert n in names, f"{n} is not declared in include/fgi.h"


def test_library_exports_flagged_entry_points(pkg):
    lib = pkg.load_library()
    for n in NAMES:
        assert hasattr(lib, n), f"libfgi.so does not export {n}"


def test_binding_declares_flagged_signatures(pkg):
    u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    sig = pkg.fgi.SIGNATURES
    assert sig["fgi_last_wave_flagged"] == [ctypes.c_void_p, u32p, u32p, ctypes.c_uint64, u64p]
    assert sig["fgi_wave_wait_flagged"] == [ctypes.c_void_p, ctypes.c_uint64, u32p, u32p, ctypes.c_uint64, u64p]
    assert hasattr(pkg.Graph, "last_wave_flagged") and hasattr(pkg.Graph, "wave_wait_flagged")


def test_version_minor_bumped(pkg):
    lib = pkg.load_library()
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.fgi_version(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) >= (0, 2)
