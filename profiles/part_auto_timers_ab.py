"""fgi_part_set_output over freshly begun slots on a two-rank in-process group with the ranks' delay timers open,
timed per collective call (host clock from the first rank's start to the last rank's return, one host thread per
rank; every rank's call ends in a device wait): `--mode plain` never opens auto-invalidation, `--mode auto` opens
it on every rank with a default delay, so every item of every call is armed. `--root` names the tree whose package
and engine are loaded, so the same script times another checkout of the project (a parent commit has only
`plain`). `--repeats` repeats the whole measurement: the spread of the medians (max - min) is the run-to-run noise
an A/B difference is read against. Prints one JSON line.

    python profiles/part_auto_timers_ab.py --mode plain --calls 20 --repeats 3 [--root DIR] [--slots 1000000]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--mode", choices=("plain", "auto"), default="plain")
    ap.add_argument("--slots", type=int, default=1_000_000)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import _pkg
    pkg = _pkg.load()
    n, P = a.slots, a.ranks
    block = -(-n // P)
    gs = [pkg.Graph(block, n_detached=0, rank=r, world=P) for r in range(P)]
    pkg.fgi.part_init_local(gs, n)
    for g in gs:
        g.part_timers_open()
        if a.mode == "auto":
            g.part_timers_auto_open(default_auto=8)
    h = np.arange(n, dtype=np.uint32)
    outs = [np.zeros(n, np.uint8) for _ in gs]
    u32, u8 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    status = [0] * P

    def one(r):
        cnt = C.c_uint64()
        status[r] = gs[r].lib.fgi_part_set_output(gs[r].h, n, h.ctypes.data_as(u32), outs[r].ctypes.data_as(u8), None, 0,
                                                  C.byref(cnt), None)

    medians, every = [], []
    version = 10
    for rep in range(a.repeats):
        ms = []
        for k in range(a.calls + 1):         # the first call of a repeat warms up
            version += 1
            pkg.fgi.part_local_run_batch(gs, [("begin_compute", h, np.full(n, version, np.uint64))])
            ts = [threading.Thread(target=one, args=(r,)) for r in range(P)]
            t0 = time.perf_counter()
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            dt = (time.perf_counter() - t0) * 1e3
            assert status == [0] * P and all(int(o.sum()) == n for o in outs), status
            if k:
                ms.append(round(dt, 4))
        medians.append(round(statistics.median(ms), 4))
        every.append(ms)
    stored = sum(g.timers_stats()["stored"] for g in gs)
    assert stored == (n if a.mode == "auto" else 0), stored
    print("PART_AUTO_TIMERS_AB " + json.dumps({
        "label": a.label, "mode": a.mode, "slots": n, "ranks": P, "calls": a.calls, "median_ms": medians,
        "spread_ms": round(max(medians) - min(medians), 4), "set_output_ms": every, "stored": stored}))
    for g in gs:
        g.close()


if __name__ == "__main__":
    main()
