"""CPU-side checks of the boundary of the auto-invalidation timers (C-ABI 0.13): the header compiles as strict C99
with the six prototypes taken by address, the 0.11 structs keep their sizes, the library exports the entry points,
the binding declares their signatures with the header's argument counts, and fgi_version says 0.13."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from test_state_view_abi import HEADER

NAMES = ["fgi_timers_auto_open", "fgi_timers_set_auto_delay", "fgi_set_output_ex", "fgi_timers_start_auto",
         "fgi_timers_auto_stats_get", "fgi_timers_list_ex"]


def test_header_library_and_binding_agree(pkg):
    names = pkg.fgi.header_symbols(HEADER)
    lib = pkg.load_library()
    for n in NAMES:
        assert n in names, f"{n} is not declared in fgi.h"
        assert hasattr(lib, n), f"libfgi.so does not export {n}"
        assert n in pkg.fgi.SIGNATURES, f"the binding declares no signature for {n}"
    for m in ("timers_auto_open", "timers_set_auto_delay", "timers_start_auto", "timers_auto_stats", "timers_list_ex"):
        assert hasattr(pkg.Graph, m), m


def test_signatures_match_the_header(pkg):
    txt = open(HEADER).read()
    for n in NAMES + ["fgi_set_output", "fgi_timers_list"]:
        m = re.search(r"fgi_status\s+" + n + r"\s*\(([^;]*)\)\s*;", txt)
        assert m, n
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len([a for a in args.split(",") if a.strip()]) == len(pkg.fgi.SIGNATURES[n]), n
    assert len(pkg.fgi.SIGNATURES["fgi_set_output_ex"]) == len(pkg.fgi.SIGNATURES["fgi_set_output"]) + 1


def test_structs_match_the_header(pkg):
    txt = open(HEADER).read()
    want = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}
    for name, struct in (("fgi_timers_auto_config", pkg.fgi.TimersAutoConfig), ("fgi_timer_auto_stats", pkg.fgi.TimerAutoStats)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S)
        assert m, name
        fields = []
        for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
            if decl.strip():
                ctype, names = decl.strip().split(None, 1)
                fields += [(x.strip(), want[ctype]) for x in names.split(",")]
        assert fields == list(struct._fields_), name
    assert ctypes.sizeof(pkg.fgi.TimersAutoConfig) == 24 and ctypes.sizeof(pkg.fgi.TimerAutoStats) == 24
    assert ctypes.sizeof(pkg.fgi.TimersConfig) == 24 and ctypes.sizeof(pkg.fgi.TimerStats) == 56


def test_header_compiles_as_c99_with_the_prototypes_taken_by_address(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "fgi.h"\n'
                   "typedef char cfg_is_24[sizeof(fgi_timers_config) == 24 ? 1 : -1];\n"
                   "typedef char stats_is_56[sizeof(fgi_timer_stats) == 56 ? 1 : -1];\n"
                   "typedef char auto_cfg_is_24[sizeof(fgi_timers_auto_config) == 24 ? 1 : -1];\n"
                   "typedef char auto_stats_is_24[sizeof(fgi_timer_auto_stats) == 24 ? 1 : -1];\n"
                   "fgi_status (*p_open)(fgi_graph*, const fgi_timers_auto_config*) = &fgi_timers_auto_open;\n"
                   "fgi_status (*p_set)(fgi_graph*, uint32_t, const uint32_t*, const uint64_t*, const uint64_t*) =\n"
                   "    &fgi_timers_set_auto_delay;\n"
                   "fgi_status (*p_out)(fgi_graph*, uint32_t, const uint32_t*, const uint8_t*, uint8_t*, uint32_t*, uint64_t,\n"
                   "                    uint64_t*, fgi_wave_stats*) = &fgi_set_output_ex;\n"
                   "fgi_status (*p_start)(fgi_graph*, uint32_t, const uint32_t*, const uint8_t*) = &fgi_timers_start_auto;\n"
                   "fgi_status (*p_stats)(fgi_graph*, fgi_timer_auto_stats*) = &fgi_timers_auto_stats_get;\n"
                   "fgi_status (*p_list)(fgi_graph*, uint32_t*, uint64_t*, uint64_t*, uint8_t*, uint64_t, uint64_t*) =\n"
                   "    &fgi_timers_list_ex;\n"
                   "int main(void) { fgi_timers_auto_config c; fgi_timer_auto_stats s; (void)c; (void)s;\n"
                   "  return p_open && p_set && p_out && p_start && p_stats && p_list ? 0 : 1; }\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.dirname(HEADER), "-c",
                        str(src), "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_version_is_0_13(pkg):
    lib = pkg.load_library()
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.fgi_version(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) >= (0, 13)
