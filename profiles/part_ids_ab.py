"""A partitioned wave's ids in the host's numbering: the device paths of fgi_part_last_wave_ids / _bits /
fgi_part_wave_ids_dev (part_out.hip; FGI_OPT_PART_IDS_PATH 1 scatter, 2 gather) against fgi_part_export_ids
(a copy of the engine-order list, a host loop through the code table and std::sort), on the same wave
(DESIGN.md §5). After profiles/part_view_wave_cost.py.

An in-process group of P ranks on ONE GPU (part_init_local), R-MAT from fgi_part_synth_rmat, labels = 1 (the
ranks' engines run on partition codes). Waves: a sparse one (16 roots), a dense one (the 4,096 slots with the
most dependants), 16 roots without dependants, and root sets of dependant-less slots sized to invalidate about
1/4096 to 1/4 of every rank's slots (a root without dependants invalidates itself alone: where the two paths
cross). Each wave runs once per round from the snapshot; then every
rank is asked, the calls interleaved round by round: setting the option drops what the accessors made, so
each timed call makes its result again. Host clock around calls that end in a stream synchronisation.
Prints one JSON line per (wave, call): the median and min-max over rounds and ranks, in ms.

    python profiles/part_ids_ab.py [--scale 20] [--ranks 2] [--rounds 9]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, path or None, method): ids_dev makes the list on the device and copies nothing but the count check
CALLS = [("ids_dev_scatter", 1, "part_wave_ids_dev"), ("ids_dev_gather", 2, "part_wave_ids_dev"),
         ("last_wave_ids_scatter", 1, "part_last_wave_ids"), ("last_wave_ids_gather", 2, "part_last_wave_ids"),
         ("last_wave_bits_scatter", 1, "part_last_wave_bits"), ("last_wave_bits_gather", 2, "part_last_wave_bits"),
         ("export_ids", None, "part_export_ids")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=9)
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
    inner = np.flatnonzero(deg > 0).astype(np.uint32)
    rng = np.random.default_rng(0x5EED0082)
    waves = {"sparse_16_roots": rng.choice(inner, 16, replace=False).astype(np.uint32),
             "dense_4096_roots": np.argsort(deg, kind="stable")[-4096:].astype(np.uint32)}
    waves["16_leaf_roots"] = leaves[:16]
    for den in (4096, 1024, 256, 64, 16, 4):
        k = min(n // den, len(leaves))
        waves[f"leaves_1/{den}"] = leaves[np.linspace(0, len(leaves) - 1, k).astype(np.int64)]
    for g in gs:
        g.snapshot()
    res = {(w, c[0]): [] for w in waves for c in CALLS}
    v_inv = {}
    for w, roots in waves.items():
        for r in range(args.rounds + 1):   # round 0 warms up (code objects, the buffers' first allocation)
            for g in gs:
                g.restore()
            stats = fgi.part_local_invalidate(gs, roots)
            v_inv[w] = [int(x.v_inv) for x in stats]
            want = [np.sort(g.part_export_ids()) for g in gs]
            for name, path, method in CALLS:
                for q, g in enumerate(gs):
                    if path is not None:
                        g.set_option(fgi.OPT_PART_IDS_PATH, path)   # forgets what the accessors made
                    t0 = time.perf_counter()
                    out = getattr(g, method)()
                    ms = (time.perf_counter() - t0) * 1e3
                    if r:
                        res[(w, name)].append(ms)
                    elif method == "part_last_wave_ids":   # results never depend on the path
                        assert np.array_equal(out, want[q]), (w, name, q)
    for (w, name), ms in res.items():
        print(json.dumps({"wave": w, "call": name, "scale": args.scale, "ranks": P, "v_inv_per_rank": v_inv[w],
                          "inv_per_n": round(sum(v_inv[w]) / n, 5), "ms_median": round(float(np.median(ms)), 4),
                          "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "samples": len(ms)}), flush=True)
    for g in gs:
        g.close()


if __name__ == "__main__":
    main()
