"""CPU-side checks of the boundary of the replica fan-out (C-ABI 0.9): the header declares fgi_subscribe,
fgi_last_wave_fanout, fgi_fanout_ids, fgi_unsubscribe_peer and fgi_sub_stats_get, the library exports them, the
binding declares their signatures with the header's argument counts, the option that pins the fan-out's source
has its number, and the statistics struct of the binding has the header's fields."""
import ctypes
import re

from test_state_view_abi import HEADER

NAMES = ["fgi_subscribe", "fgi_last_wave_fanout", "fgi_fanout_ids", "fgi_unsubscribe_peer", "fgi_sub_stats_get"]


def test_header_library_and_binding_agree(pkg):
    names = pkg.fgi.header_symbols(HEADER)
    lib = pkg.load_library()
    for n in NAMES:
        assert n in names, f"{n} is not declared in fgi.h"
        assert hasattr(lib, n), f"libfgi.so does not export {n}"
        assert n in pkg.fgi.SIGNATURES, f"the binding declares no signature for {n}"
    txt = open(HEADER).read()
    assert "#define FGI_OPT_FANOUT_PATH 20" in txt and pkg.fgi.OPT_FANOUT_PATH == 20
    assert "#define FGI_MAX_PEERS 4096u" in txt and pkg.fgi.MAX_PEERS == 4096
    assert "#define FGI_SUB_ADDED 0u" in txt and "#define FGI_SUB_INVALIDATED 1u" in txt
    assert (pkg.fgi.SUB_ADDED, pkg.fgi.SUB_INVALIDATED) == (0, 1)
    for m in ("subscribe", "last_wave_fanout", "fanout_ids", "unsubscribe_peer", "sub_stats"):
        assert hasattr(pkg.Graph, m), m


def test_signatures_match_the_header(pkg):
    """The argument counts of the binding against the header's declarations (a mismatch would corrupt the
    call, not fail it)."""
    txt = open(HEADER).read()
    for n in NAMES:
        m = re.search(r"fgi_status\s+" + n + r"\s*\(([^;]*)\)\s*;", txt)
        assert m, n
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len([a for a in args.split(",") if a.strip()]) == len(pkg.fgi.SIGNATURES[n]), n


def test_stats_struct_matches_the_header(pkg):
    txt = open(HEADER).read()
    m = re.search(r"typedef struct fgi_sub_stats \{(.*?)\} fgi_sub_stats;", txt, flags=re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(x.strip(), ctype) for x in names.split(",")]
    want = {"uint64_t": ctypes.c_uint64, "double": ctypes.c_double}
    assert [(k, want[t]) for k, t in fields] == list(pkg.fgi.SubStats._fields_)


def test_version_is_0_9(pkg):
    lib = pkg.load_library()
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.fgi_version(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) >= (0, 9)
