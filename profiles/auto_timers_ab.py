"""fgi_set_output over freshly begun slots with the delay timers open, timed per call (host clock around the call,
which ends in a device wait): `--mode plain` never opens auto-invalidation, `--mode auto` opens it with a default
delay, so every item of every call is armed. `--root` names the tree whose package and engine are loaded, so the
same script times another checkout of the project (a parent commit has only `plain`). Prints one JSON line.

    python profiles/auto_timers_ab.py --mode plain --runs 5 [--root DIR] [--slots 1000000]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--mode", choices=("plain", "auto"), default="plain")
    ap.add_argument("--slots", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import _pkg
    pkg = _pkg.load()
    n = a.slots
    g = pkg.Graph(n)
    g.timers_open()
    if a.mode == "auto":
        g.timers_auto_open(default_auto=8)
    h = np.arange(n, dtype=np.uint32)
    out = np.zeros(n, np.uint8)
    cnt = C.c_uint64()
    u32, u8 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    ms = []
    for r in range(a.runs + 1):          # the first run warms up
        g.begin_compute(h, np.full(n, 10 + r, np.uint64))
        t0 = time.perf_counter()
        st = g.lib.fgi_set_output(g.h, n, h.ctypes.data_as(u32), out.ctypes.data_as(u8), None, 0, C.byref(cnt), None)
        dt = (time.perf_counter() - t0) * 1e3
        assert st == 0 and int(out.sum()) == n
        if r:
            ms.append(round(dt, 4))
    stored = g.timers_stats()["stored"]
    assert stored == (n if a.mode == "auto" else 0), stored
    print("AUTO_TIMERS_AB " + json.dumps({"label": a.label, "mode": a.mode, "slots": n, "set_output_ms": ms, "stored": stored}))


if __name__ == "__main__":
    main()
