"""CPU-side checks of the boundary of the delay timers per rank of a partition (C-ABI 0.12): the header declares
fgi_part_timers_open, _set_delay, _run_due, _fired_detached and fgi_part_local_timers_run_due, the library
exports them, the binding declares their signatures with the header's argument counts and the Graph methods,
the header still compiles as strict C99, and fgi_version says 0.12."""
import ctypes
import os
import re
import shutil
import subprocess

from test_state_view_abi import HEADER

NAMES = ["fgi_part_timers_open", "fgi_part_timers_set_delay", "fgi_part_timers_run_due",
         "fgi_part_timers_fired_detached", "fgi_part_local_timers_run_due"]
ARGS = {"fgi_part_timers_open": 2, "fgi_part_timers_set_delay": 4, "fgi_part_timers_run_due": 8,
        "fgi_part_timers_fired_detached": 4, "fgi_part_local_timers_run_due": 6}


def test_header_library_and_binding_agree(pkg):
    names = pkg.fgi.header_symbols(HEADER)
    lib = pkg.load_library()
    for n in NAMES:
        assert n in names, f"{n} is not declared in fgi.h"
        assert hasattr(lib, n), f"libfgi.so does not export {n}"
        assert n in pkg.fgi.SIGNATURES, f"the binding declares no signature for {n}"
    for m in ("part_timers_open", "part_timers_set_delay", "part_timers_run_due", "part_timers_fired_detached"):
        assert callable(getattr(pkg.Graph, m, None)), m
    assert callable(getattr(pkg.fgi, "part_local_timers_run_due", None))


def test_signatures_match_the_header(pkg):
    """The argument counts of the binding against the header's declarations (a mismatch would corrupt the
    call, not fail it), and both against the counts the issue's prototypes have."""
    txt = open(HEADER).read()
    for n in NAMES:
        m = re.search(r"fgi_status\s+" + n + r"\s*\(([^;]*)\)\s*;", txt)
        assert m, n
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        count = len([a for a in args.split(",") if a.strip()])
        assert count == len(pkg.fgi.SIGNATURES[n]) == ARGS[n], (n, count, len(pkg.fgi.SIGNATURES[n]))


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    assert shutil.which(cc), "no C compiler to check the header with"
    src = tmp_path / "t.c"
    src.write_text('#include "fgi.h"\n'
                   "int main(void) {\n"
                   "  fgi_status (*open_)(fgi_graph*, const fgi_timers_config*) = &fgi_part_timers_open;\n"
                   "  fgi_status (*tick)(fgi_graph*, uint64_t, uint32_t*, uint64_t, uint64_t*, uint64_t*, uint64_t*,\n"
                   "                     fgi_wave_stats*) = &fgi_part_timers_run_due;\n"
                   "  fgi_status (*all)(fgi_graph* const*, uint32_t, uint64_t, uint64_t*, uint64_t*, fgi_wave_stats*) =\n"
                   "      &fgi_part_local_timers_run_due;\n"
                   "  return open_ != 0 && tick != 0 && all != 0 && &fgi_part_timers_set_delay != 0 &&\n"
                   "         &fgi_part_timers_fired_detached != 0 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-Wno-address", "-I",
                        os.path.dirname(HEADER), "-c", str(src), "-o", str(tmp_path / "t.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_version_is_0_12(pkg):
    lib = pkg.load_library()
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.fgi_version(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) >= (0, 12)
