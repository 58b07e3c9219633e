"""A partition rank's fan-out (fgi_part_last_wave_fanout; fanout.hip) by the form of its source,
on the same wave with the same subscriptions:
  (a) probe   FGI_OPT_FANOUT_PATH 2, nothing made before: k_fo_probe writes inv & has from the subscribed handles
  (b) gather  FGI_OPT_FANOUT_PATH 3 with FGI_OPT_PART_IDS_PATH 2: part_out_bits' k_pout_gather renumbers the whole
              bitmap inside the call, then the join ANDs it with has
  (c) list    FGI_OPT_FANOUT_PATH 1: the rank's ascending ids (part_out_ids, made inside the call), the list form

An in-process group of P ranks on ONE GPU, R-MAT from fgi_part_synth_rmat, labels = 1 (partition codes). One
dense wave (the 4,096 slots with the most dependants) per round from the snapshot; a fan-out is one-shot, so a
round measures one form and the delivered entries are subscribed again; the forms alternate round by round.
kernel_ms: fgi_sub_stats.last_kernel_ms of the call (HIP events: the kernels that make the source inside the
call plus the join's kernels, for every form). call_ms: host clock around the fan-out call that makes the lists
(no list is copied). One JSON line per form: medians and min-max over rounds and ranks.

    python profiles/part_fanout_ab.py [--scale 20] [--ranks 2] [--rounds 20] [--subs 1000000] [--peers 100]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ["probe", "gather", "list"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--subs", type=int, default=1000000)
    ap.add_argument("--peers", type=int, default=100)
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
    roots = np.argsort(deg, kind="stable")[-4096:].astype(np.uint32)
    rng = np.random.default_rng(0x5EED0091)
    sh = rng.integers(0, n, args.subs).astype(np.uint32)
    sp = rng.integers(0, args.peers, args.subs).astype(np.uint32)
    sc = np.arange(args.subs, dtype=np.uint64)
    for g in gs:
        g.snapshot()
    own = [sh // block == r for r in range(P)]
    for r, g in enumerate(gs):   # each rank its own share
        assert not g.part_subscribe(sh[own[r]], sp[own[r]], sc[own[r]]).any()
    res = {f: {"kernel_ms": [], "call_ms": []} for f in FORMS}
    fan_path = {"probe": 2, "gather": 3, "list": 1}
    off = np.zeros(args.peers + 1, np.uint64)
    offp = off.ctypes.data_as(C.POINTER(C.c_uint64))
    v_inv, delivered = None, None
    for rnd in range(len(FORMS) * (args.rounds + 1)):   # the first round of each form warms up
        form = FORMS[rnd % len(FORMS)]
        stats = fgi.part_local_invalidate(gs, roots)
        v_inv = [int(x.v_inv) for x in stats]
        got = []
        for r, g in enumerate(gs):
            g.set_option(fgi.OPT_PART_IDS_PATH, 2 if form == "gather" else 0)   # forgets what the accessors made
            g.set_option(fgi.OPT_FANOUT_PATH, fan_path[form])
            cnt = C.c_uint64()
            t0 = time.perf_counter()
            st = g.lib.fgi_part_last_wave_fanout(g.h, args.peers, offp, None, None, 0, C.byref(cnt))
            ms = (time.perf_counter() - t0) * 1e3
            assert st == fgi.OK, st
            got.append(int(cnt.value))
            if rnd >= len(FORMS):
                res[form]["kernel_ms"].append(g.sub_stats()["last_kernel_ms"])
                res[form]["call_ms"].append(ms)
        ids = [g.part_last_wave_ids() for g in gs]
        hit = [own[r] & np.isin(sh, ids[r]) for r in range(P)]
        assert got == [int(h.sum()) for h in hit], (form, got)   # results never depend on the form
        delivered = got
        for r, g in enumerate(gs):   # the graph as before the wave, the delivered entries stored again
            g.restore()
            assert not g.part_subscribe(sh[hit[r]], sp[hit[r]], sc[hit[r]]).any()

    def summary(x):
        return {"median": round(float(np.median(x)), 4), "min": round(min(x), 4), "max": round(max(x), 4)}

    for form in FORMS:
        print(json.dumps({"form": form, "scale": args.scale, "ranks": P, "subs": args.subs, "peers": args.peers,
                          "v_inv_per_rank": v_inv, "delivered_per_rank": delivered,
                          "kernel_ms": summary(res[form]["kernel_ms"]), "call_ms": summary(res[form]["call_ms"]),
                          "samples": len(res[form]["kernel_ms"])}),
              flush=True)
    for g in gs:
        g.close()


if __name__ == "__main__":
    main()
