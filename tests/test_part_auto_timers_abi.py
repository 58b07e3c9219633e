"""CPU-side checks of the boundary of the auto-invalidation timers per rank of a partition (C-ABI 0.14): the
library exports the six entry points, the header declares them and compiles as strict C99 with the six prototypes
taken by address, the binding declares their signatures with the header's argument counts, each mirrors its 0.13
call's signature, and fgi_version says 0.14."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from test_state_view_abi import HEADER

NAMES = ["fgi_part_timers_auto_open", "fgi_part_timers_set_auto_delay", "fgi_part_set_output_ex", "fgi_part_timers_start_auto",
         "fgi_part_timers_auto_stats_get", "fgi_part_timers_list_ex"]
# the 0.13 call each one is, per rank
SINGLE = {"fgi_part_timers_auto_open": "fgi_timers_auto_open", "fgi_part_timers_set_auto_delay": "fgi_timers_set_auto_delay",
          "fgi_part_set_output_ex": "fgi_set_output_ex", "fgi_part_timers_start_auto": "fgi_timers_start_auto",
          "fgi_part_timers_auto_stats_get": "fgi_timers_auto_stats_get", "fgi_part_timers_list_ex": "fgi_timers_list_ex"}


def test_header_library_and_binding_agree(pkg):
    names = pkg.fgi.header_symbols(HEADER)
    lib = pkg.load_library()
    for n in NAMES:
        assert n in names, f"{n} is not declared in fgi.h"
        assert hasattr(lib, n), f"libfgi.so does not export {n}"
        assert n in pkg.fgi.SIGNATURES, f"the binding declares no signature for {n}"
    for m in ("part_timers_auto_open", "part_timers_set_auto_delay", "part_timers_start_auto", "part_timers_auto_stats",
              "part_timers_list_ex"):
        assert hasattr(pkg.Graph, m), m


def test_signatures_match_the_header(pkg):
    txt = open(HEADER).read()
    for n in NAMES + ["fgi_part_set_output"]:
        m = re.search(r"fgi_status\s+" + n + r"\s*\(([^;]*)\)\s*;", txt)
        assert m, n
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len([a for a in args.split(",") if a.strip()]) == len(pkg.fgi.SIGNATURES[n]), n
    for n, one in SINGLE.items():
        assert pkg.fgi.SIGNATURES[n] == pkg.fgi.SIGNATURES[one], (n, one)
    assert len(pkg.fgi.SIGNATURES["fgi_part_set_output_ex"]) == len(pkg.fgi.SIGNATURES["fgi_part_set_output"]) + 1


def test_part_set_output_takes_transient_flags(pkg):
    import inspect
    p = inspect.signature(pkg.Graph.part_set_output).parameters
    assert "transient" in p and p["transient"].default is None


def test_the_0_13_section_points_to_the_ranks_calls():
    txt = open(HEADER).read()
    at = txt.index("C-ABI 0.13;")
    section = txt[at:txt.index("typedef struct fgi_timers_auto_config", at)]
    assert "Single device only" not in section and "0.14" in section and "fgi_part_" in section


def test_header_compiles_as_c99_with_the_prototypes_taken_by_address(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "fgi.h"\n'
                   "typedef char auto_cfg_is_24[sizeof(fgi_timers_auto_config) == 24 ? 1 : -1];\n"
                   "typedef char auto_stats_is_24[sizeof(fgi_timer_auto_stats) == 24 ? 1 : -1];\n"
                   "fgi_status (*p_open)(fgi_graph*, const fgi_timers_auto_config*) = &fgi_part_timers_auto_open;\n"
                   "fgi_status (*p_set)(fgi_graph*, uint32_t, const uint32_t*, const uint64_t*, const uint64_t*) =\n"
                   "    &fgi_part_timers_set_auto_delay;\n"
                   "fgi_status (*p_out)(fgi_graph*, uint32_t, const uint32_t*, const uint8_t*, uint8_t*, uint32_t*, uint64_t,\n"
                   "                    uint64_t*, fgi_wave_stats*) = &fgi_part_set_output_ex;\n"
                   "fgi_status (*p_start)(fgi_graph*, uint32_t, const uint32_t*, const uint8_t*) = &fgi_part_timers_start_auto;\n"
                   "fgi_status (*p_stats)(fgi_graph*, fgi_timer_auto_stats*) = &fgi_part_timers_auto_stats_get;\n"
                   "fgi_status (*p_list)(fgi_graph*, uint32_t*, uint64_t*, uint64_t*, uint8_t*, uint64_t, uint64_t*) =\n"
                   "    &fgi_part_timers_list_ex;\n"
                   "int main(void) { return p_open && p_set && p_out && p_start && p_stats && p_list ? 0 : 1; }\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.dirname(HEADER), "-c",
                        str(src), "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_version_is_0_14(pkg):
    lib = pkg.load_library()
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.fgi_version(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) >= (0, 14)
