"""Wave cost of a partition with the per-rank state view open against closed, and the scatter / gather
crossover of k_view_part_wave. After profiles/view_wave_cost.py.

An in-process group of P ranks on ONE GPU (part_init_local), R-MAT from fgi_part_synth_rmat, labels = 1 (the
ranks' engines run on partition codes). Waves: a dense one (the 64 slots with the most dependants), one from
16 roots without dependants, and root sets of dependant-less slots sized to invalidate about 1/256, 1/64,
1/16 and 1/4 of every rank's slots (a root without dependants invalidates itself alone, so the set's size is
the wave's). For each wave: view closed, then open with FGI_OPT_PART_VIEW_PATH pinned to scatter, pinned to
gather, and auto, interleaved round by round; every wave starts from the snapshot (fgi_restore, untimed; with
a view open it rebuilds the planes). Prints one JSON line per (wave, state): the median and min-max wall time
of the group call in ms (shared-GPU wall time: the ranks' kernels share one device), the median over rounds
of the ranks' mean kernel_ms (per-rank kernel time), and the plane words the ranks published.

    python profiles/part_view_wave_cost.py [--scale 24] [--ranks 2] [--rounds 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATES = [("closed", None), ("scatter", 1), ("gather", 2), ("auto", 0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=24)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--edge-factor", type=int, default=16)
    args = ap.parse_args()
    import _pkg
    pkg = _pkg.load()
    fgi = pkg.fgi
    P, n = args.ranks, 1 << args.scale
    block = -(-n // P)
    gs = [pkg.Graph(block, rank=r, world=P, labels=1) for r in range(P)]
    fgi.part_init_local(gs, n)
    for g in gs:
        g.part_synth_rmat(args.scale, args.edge_factor, 0x5EED0081, 0, 0)
    deg = np.concatenate([g.degrees()[0][:min(block, n - r * block)] for r, g in enumerate(gs)])
    leaves = np.flatnonzero(deg == 0).astype(np.uint32)
    waves = {"dense_64_hubs": np.argsort(deg, kind="stable")[-64:].astype(np.uint32), "16_leaf_roots": leaves[:16]}
    for den in (256, 64, 16, 4):
        k = min(n // den, len(leaves))
        waves[f"leaves_1/{den}"] = leaves[np.linspace(0, len(leaves) - 1, k).astype(np.int64)]
    for g in gs:
        g.snapshot()
    res = {(w, s): {"ms": [], "kernel_ms": [], "words": [], "v_inv": 0} for w in waves for s, _ in STATES}
    for w, roots in waves.items():
        for r in range(args.rounds + 1):   # round 0 warms up (and learns the wave's plan)
            for state, path in STATES:
                for g in gs:
                    if path is not None:
                        g.set_option(fgi.OPT_PART_VIEW_PATH, path)
                        g.part_open_state_view()
                    g.restore()
                before = sum(g.view_stats().words_published for g in gs)
                t0 = time.perf_counter()
                stats = fgi.part_local_invalidate(gs, roots)
                ms = (time.perf_counter() - t0) * 1e3
                if r:
                    e = res[(w, state)]
                    e["ms"].append(ms)
                    e["kernel_ms"].append(float(np.mean([x.kernel_ms for x in stats])))
                    e["words"].append(int(sum(g.view_stats().words_published for g in gs) - before))
                    e["v_inv"] = int(sum(x.v_inv for x in stats))
                if path is not None:
                    for g in gs:
                        g.close_state_view()
    for (w, s), e in res.items():
        print(json.dumps({"wave": w, "view": s, "scale": args.scale, "ranks": P, "v_inv": e["v_inv"],
                          "inv_per_n": round(e["v_inv"] / n, 5),
                          "call_ms_median": round(float(np.median(e["ms"])), 4),
                          "call_ms_min": round(min(e["ms"]), 4), "call_ms_max": round(max(e["ms"]), 4),
                          "rank_kernel_ms_median": round(float(np.median(e["kernel_ms"])), 4),
                          "words_published": sorted(set(e["words"])), "rounds": args.rounds}), flush=True)
    for g in gs:
        g.close()


if __name__ == "__main__":
    main()
