"""Wave cost with the host-memory state view open against closed: configs[1] (R-MAT 24,
4,096 degree-weighted roots) through fgi_invalidate_bits, a 16-root wave on the same graph (the first 16 of
those roots: they reach the same giant component, so that wave is dense too), and a wave from 16 roots
without dependants (each invalidates itself alone: the cost of a wave that changes a few words). One graph,
one session, the two states interleaved; every wave starts from the snapshot (fgi_restore, untimed; with the
view open it rebuilds the planes). Prints one JSON line per (wave, state): the median and min-max wall time
of the call in ms, the wave's kernel time, and the plane words the wave published.

    python profiles/view_wave_cost.py [--scale 24] [--rounds 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import _pkg
    pkg = _pkg.load()
    from stl_fusion_amd import workloads as W
    cfg = dict(W.CONFIGS["rmat24"])
    cfg["scale"] = args.scale
    g = pkg.Graph(W.n_slots(cfg))
    W.build(g, cfg)
    roots = {"4096_roots": W.roots_for(g, cfg)}
    roots["16_roots"] = roots["4096_roots"][:16].copy()
    deg, _ = g.degrees()
    roots["16_leaf_roots"] = np.nonzero(deg[:W.n_slots(cfg)] == 0)[0][:16].astype(np.uint32)
    g.snapshot()
    res = {(w, s): {"ms": [], "kernel_ms": [], "words": [], "v_inv": 0} for w in roots for s in ("closed", "open")}
    # one wave kind at a time (a wave's first level group is sized from the wave before it, so mixing kinds
    # would make every wave pay a second group); round 0 of each kind warms up
    for w, rs in roots.items():
        for r in range(args.rounds + 1):
            for state in ("closed", "open"):
                if state == "open":
                    g.open_state_view()
                g.restore()
                before = g.view_stats().words_published
                ws = pkg.WaveStats()
                t0 = time.perf_counter()
                _, v = g.invalidate_bits(rs, stats=ws)
                ms = (time.perf_counter() - t0) * 1e3
                if r:
                    e = res[(w, state)]
                    e["ms"].append(ms)
                    e["kernel_ms"].append(ws.kernel_ms)
                    e["words"].append(int(g.view_stats().words_published - before))
                    e["v_inv"] = int(v)
                if state == "open":
                    g.close_state_view()
    for (w, s), e in res.items():
        print(json.dumps({"wave": w, "view": s, "scale": args.scale, "v_inv": e["v_inv"],
                          "call_ms_median": round(float(np.median(e["ms"])), 4),
                          "call_ms_min": round(min(e["ms"]), 4), "call_ms_max": round(max(e["ms"]), 4),
                          "kernel_ms_median": round(float(np.median(e["kernel_ms"])), 4),
                          "words_published": sorted(set(e["words"])), "rounds": args.rounds}))


if __name__ == "__main__":
    main()
