"""CPU-side checks of the boundary of a partition's host-facing wave (C-ABI 0.8): the header declares
fgi_part_invalidate_host, fgi_part_invalidate_bits, fgi_part_last_wave_ids, fgi_part_last_wave_bits and
fgi_part_wave_ids_dev, the library exports them, the binding declares their signatures, and the option that
pins the path of their device-side renumbering has its number."""
import ctypes

from test_state_view_abi import HEADER

NAMES = ["fgi_part_invalidate_host", "fgi_part_invalidate_bits", "fgi_part_last_wave_ids", "fgi_part_last_wave_bits",
         "fgi_part_wave_ids_dev"]


def test_header_library_and_binding_agree(pkg):
    names = pkg.fgi.header_symbols(HEADER)
    lib = pkg.load_library()
    for n in NAMES:
        assert n in names, f"{n} is not declared in fgi.h"
        assert hasattr(lib, n), f"libfgi.so does not export {n}"
        assert n in pkg.fgi.SIGNATURES, f"the binding declares no signature for {n}"
    assert "#define FGI_OPT_PART_IDS_PATH 19" in open(HEADER).read() and pkg.fgi.OPT_PART_IDS_PATH == 19
    for m in ("part_invalidate_host", "part_last_wave_ids", "part_last_wave_bits", "part_wave_ids_dev"):
        assert hasattr(pkg.Graph, m), m


def test_signatures_match_the_header(pkg):
    """The argument counts of the binding against the header's declarations (a mismatch would corrupt the
    call, not fail it)."""
    import re
    txt = open(HEADER).read()
    for n in NAMES:
        m = re.search(r"fgi_status\s+" + n + r"\s*\(([^;]*)\)\s*;", txt)
        assert m, n
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len([a for a in args.split(",") if a.strip()]) == len(pkg.fgi.SIGNATURES[n]), n


def test_version_is_0_8(pkg):
    lib = pkg.load_library()
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.fgi_version(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) >= (0, 8)
