"""What the delay timers per rank of a partition (fgi_part_timers_*; timers.hip) save a multi-GPU
host: one wave plus the tick that fires what the wave started, two ways, on the same graph with the same roots.
  (a) host    the path the feature replaces, on a group without timers: after the wave every rank downloads
              fgi_part_last_flagged, the host keeps (slot, due) of the records carrying DelayStarted, picks the due
              slots of all ranks at the tick and calls fgi_part_invalidate_host on every rank. The host's map is
              two numpy arrays and the pick one mask, and nothing is re-checked per node: the cheapest host there is.
  (b) device  fgi_part_local_timers_run_due on a group whose ranks opened timers (default delay 5).

An in-process group of P ranks on ONE GPU per side, R-MAT from host arrays (the nodes need state flags), 10 % of
the slots with an InvalidationDelay, 1,024 roots. A round restores the snapshot (outside the timed window), sets
the clock, then times wave + tick with a host clock, the window closed by a device synchronise on both sides
(the tick's own arming kernel is queued behind its wave). One group is alive at a time: the sides alternate block
by block (--blocks of them each, a fresh group per block, its first round warms up), because with both groups
alive the one made second runs the same round about 2 ms slower, whichever side it is (--together 1 measures
that, four graphs and their streams in one process; profiles/part_timers.json holds both orders). One JSON line per side with the median and the min-max over all
its rounds, then one with the ratio.

--split 1 adds a device synchronise between the wave and the tick and reports the parts as well: the wave's call,
what was still queued behind it when it returned (the flagged-set pass, and on the device side the arming
kernel), and the tick (the sum is then not the headline number: the tick no longer overlaps the wave's tail).
--first names the side whose group is made first.

    python profiles/part_timers_ab.py [--scale 20] [--ranks 2] [--rounds 7] [--blocks 2] [--delayed-pct 10]
                                      [--split 0] [--first host] [--together 0]
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

CONSISTENT, F_DS, F_HD = 1, 8, 16
DELAY = 5


def each_rank(gs, fn):
    out, err = [None] * len(gs), []

    def run(r):
        try:
            out[r] = fn(r, gs[r])
        except Exception as e:   # noqa: BLE001
            err.append((r, e))
    ts = [threading.Thread(target=run, args=(r,)) for r in range(len(gs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not err, err
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--delayed-pct", type=int, default=10)
    ap.add_argument("--split", type=int, default=0)
    ap.add_argument("--first", choices=("host", "device"), default="host")
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--together", type=int, default=0)
    args = ap.parse_args()
    import torch
    import _pkg
    import fgo as O
    pkg = _pkg.load()
    fgi = pkg.fgi
    from stl_fusion_amd.workloads import pick_roots
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.cuda.set_device(0)
    P, n, seed = args.ranks, 1 << args.scale, 0x5EED0027
    block = -(-n // P)
    rng = np.random.default_rng(21)
    versions = O.version_of(seed, np.arange(n, dtype=np.uint64)).copy()
    flags = np.full(n, CONSISTENT, np.uint32)
    flags[rng.random(n) < args.delayed_pct / 100.0] |= F_HD
    s, d = O.gen_rmat(args.scale, args.edge_factor, seed)
    tags = versions[d]
    slots = np.arange(n, dtype=np.uint32)
    roots = pick_roots(1024, n, 0x5EED1027, np.ones(n, np.uint8))

    def group(timers):
        gs = [pkg.Graph(block, rank=r, world=P) for r in range(P)]
        fgi.part_init_local(gs, n)
        for g in gs:
            g.part_register_nodes(slots, versions, flags)
            g.part_load_edges(s, d, tags)
            if timers:
                g.part_timers_open(default_delay=DELAY)
            g.snapshot()
        return gs
    order = ("host", "device") if args.first == "host" else ("device", "host")
    ms = {k: [] for k in order}
    wave_ms = {k: [] for k in order}
    call_ms = {k: [] for k in order}
    shape = {}

    def one_round(side, gs, now, timed):
        for g in gs:
            g.restore()
            if side == "device":
                g.timers_set_now(now)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st1 = fgi.part_local_invalidate(gs, roots)
        if args.split:
            tc = time.perf_counter()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
        if side == "host":
            held_s, held_t = [], []
            for g in gs:
                _, ids, fl = g.part_last_flagged()
                started = (fl & F_DS) != 0
                held_s.append(ids[started])
                held_t.append(np.full(int(started.sum()), now + DELAY, np.uint64))
            hs, ht = np.concatenate(held_s), np.concatenate(held_t)
            due = np.sort(hs[ht <= now + DELAY])
            ones = np.ones(len(due), np.uint8)
            each_rank(gs, lambda r, g: g.part_invalidate_host(due, ones, want=None))
            fired = len(due)
        else:
            per, _, _ = fgi.part_local_timers_run_due(gs, now + DELAY)
            fired = sum(per)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        got = dict(v_inv_wave=sum(int(x.v_inv) for x in st1), fired=int(fired),
                   v_inv_tick=sum(len(g.part_last_wave_ids()) for g in gs))
        shape.setdefault(side, got)
        assert shape[side] == got and got == shape[order[0]], (side, got, shape)   # both sides do the same work
        if timed:
            ms[side].append(dt)
            if args.split:
                wave_ms[side].append((t1 - t0) * 1e3)
                call_ms[side].append((tc - t0) * 1e3)

    if args.together:   # both groups alive, the sides alternating round by round
        sides = {side: group(side == "device") for side in order}
        for rnd in range(2 * (args.rounds + 1)):
            side = order[rnd % 2]
            one_round(side, sides[side], 10 * (rnd // 2), rnd >= 2)
        for gs in sides.values():
            for g in gs:
                g.close()
    else:               # one group alive at a time, the sides alternating block by block
        for blk in range(args.blocks):
            for side in order:
                gs = group(side == "device")
                for rnd in range(args.rounds + 1):
                    one_round(side, gs, 10 * rnd, rnd >= 1)
                for g in gs:
                    g.close()
                del gs

    def summary(x):
        return {"median": round(float(np.median(x)), 4), "min": round(min(x), 4), "max": round(max(x), 4)}
    for side in ("host", "device"):
        print(json.dumps({"side": side, "scale": args.scale, "ranks": P, "delayed_pct": args.delayed_pct, "roots": len(roots),
                          **shape[side], "wave_plus_tick_ms": summary(ms[side]), "samples": len(ms[side]),
                          "first": args.first, "together": args.together,
                          **({"split": 1, "wave_ms": summary(wave_ms[side]), "wave_call_ms": summary(call_ms[side]),
                              "wave_tail_ms": summary([a - b for a, b in zip(wave_ms[side], call_ms[side])]),
                              "tick_ms": summary([a - b for a, b in zip(ms[side], wave_ms[side])])} if args.split else {})}),
              flush=True)
    print(json.dumps({"host_over_device": round(float(np.median(ms["host"]) / np.median(ms["device"])), 3)}), flush=True)


if __name__ == "__main__":
    main()
