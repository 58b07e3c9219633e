"""CPU-side checks of the boundary of the delay timers (C-ABI 0.11): the header compiles as C99 with the new
section and its structs have the declared sizes, the library exports the entry points, the binding declares
their signatures with the header's argument counts, and fgi_version says 0.11."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from test_state_view_abi import HEADER

NAMES = ["fgi_timers_open", "fgi_timers_close", "fgi_timers_set_delay", "fgi_timers_set_now", "fgi_timers_run_due",
         "fgi_timers_next_due", "fgi_timers_stats_get", "fgi_timers_list"]


def test_header_library_and_binding_agree(pkg):
    names = pkg.fgi.header_symbols(HEADER)
    lib = pkg.load_library()
    for n in NAMES:
        assert n in names, f"{n} is not declared in fgi.h"
        assert hasattr(lib, n), f"libfgi.so does not export {n}"
        assert n in pkg.fgi.SIGNATURES, f"the binding declares no signature for {n}"
    txt = open(HEADER).read()
    assert "#define FGI_TIMER_NEVER 0xFFFFFFFFFFFFFFFFull" in txt and "#define FGI_TIMER_NONE 0xFFFFFFFFFFFFFFFFull" in txt
    assert pkg.fgi.TIMER_NEVER == pkg.fgi.TIMER_NONE == 2 ** 64 - 1
    for m in ("timers_open", "timers_set_delay", "timers_set_now", "timers_run_due", "timers_next_due", "timers_stats",
              "timers_list"):
        assert hasattr(pkg.Graph, m), m


def test_signatures_match_the_header(pkg):
    txt = open(HEADER).read()
    for n in NAMES:
        m = re.search(r"fgi_status\s+" + n + r"\s*\(([^;]*)\)\s*;", txt)
        assert m, n
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len([a for a in args.split(",") if a.strip()]) == len(pkg.fgi.SIGNATURES[n]), n


def test_structs_match_the_header(pkg):
    txt = open(HEADER).read()
    want = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}
    for name, struct in (("fgi_timers_config", pkg.fgi.TimersConfig), ("fgi_timer_stats", pkg.fgi.TimerStats)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S)
        assert m, name
        fields = []
        for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
            if decl.strip():
                ctype, names = decl.strip().split(None, 1)
                fields += [(x.strip(), want[ctype]) for x in names.split(",")]
        assert fields == list(struct._fields_), name
    assert ctypes.sizeof(pkg.fgi.TimersConfig) == 24 and ctypes.sizeof(pkg.fgi.TimerStats) == 56


def test_header_compiles_as_c99_with_the_declared_sizes(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "fgi.h"\n'
                   "typedef char cfg_is_24[sizeof(fgi_timers_config) == 24 ? 1 : -1];\n"
                   "typedef char stats_is_56[sizeof(fgi_timer_stats) == 56 ? 1 : -1];\n"
                   "int main(void) { fgi_timers_config c; fgi_timer_stats s; unsigned long long n = FGI_TIMER_NEVER;\n"
                   "  (void)c; (void)s; return n == FGI_TIMER_NONE && &fgi_timers_run_due != 0 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-Wno-address", "-I",
                        os.path.dirname(HEADER), "-c", str(src), "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_version_is_0_11(pkg):
    lib = pkg.load_library()
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.fgi_version(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) >= (0, 11)
