"""Load time of a partition from per-rank shards against the replicated calls: the same R-MAT
edge list and node list into a fresh in-process P-rank group on one GPU (both ranks share the device, and the
transport is device copies between the group's buffers, not xGMI).
  replicated: every rank is given every node and every edge (fgi_part_register_nodes / fgi_part_load_edges),
              rank after rank; wall time per rank.
  sharded:    rank r is given nodes r::P and edges r::P (fgi_part_local_register_shards /
              fgi_part_local_load_shards, one host thread per rank); wall time of the call = every rank's.
Then one wave from 64 roots, whose invalidated count is printed so that the paths can be compared. Run under
`rocprofv3 --kernel-trace --stats` for the per-kernel table (k_shard_count, k_shard_scatter). The replicated
mode uses nothing the sharded calls added, so the script also runs on the tree before them.
Usage: python profiles/part_shard_load.py replicated|sharded [scale=20] [edge factor=16] [P=2] [labels=0]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _pkg  # noqa: E402
import fgo as O  # noqa: E402

pkg = _pkg.load()


def main():
    mode = sys.argv[1]
    scale = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    ef = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    P = int(sys.argv[4]) if len(sys.argv) > 4 else 2
    labels = int(sys.argv[5]) if len(sys.argv) > 5 else 0
    seed = 0x5EED0027
    n = 1 << scale
    slots = np.arange(n, dtype=np.uint32)
    versions = O.version_of(seed, np.arange(n, dtype=np.uint64)).copy()
    s, d = O.gen_rmat(scale, ef, seed)
    tags = versions[d]
    block = -(-n // P)
    gs = [pkg.Graph(block, rank=r, world=P, labels=labels) for r in range(P)]
    pkg.fgi.part_init_local(gs, n)
    reg, load = [], []
    if mode == "replicated":
        for g in gs:
            t0 = time.perf_counter()
            g.part_register_nodes(slots, versions)
            t1 = time.perf_counter()
            g.part_load_edges(s, d, tags)
            t2 = time.perf_counter()
            reg.append(t1 - t0)
            load.append(t2 - t1)
    else:
        nodes = [(slots[r::P].copy(), versions[r::P].copy()) for r in range(P)]
        edges = [(s[r::P].copy(), d[r::P].copy(), tags[r::P].copy()) for r in range(P)]
        t0 = time.perf_counter()
        pkg.fgi.part_local_register_shards(gs, nodes)
        t1 = time.perf_counter()
        pkg.fgi.part_local_load_shards(gs, edges)
        t2 = time.perf_counter()
        reg, load = [t1 - t0] * P, [t2 - t1] * P
    roots = O.gen_roots(64, n, 0x5EED1027, np.bincount(s, minlength=n))
    stats = pkg.fgi.part_local_invalidate(gs, roots)
    print(f"{mode} scale {scale} ef {ef} P {P} labels {labels}: register s/rank " +
          " ".join(f"{x:.3f}" for x in reg) + " | load_edges s/rank " + " ".join(f"{x:.3f}" for x in load) +
          f" | wave v_inv {sum(x.v_inv for x in stats)} e_trav {sum(x.e_trav for x in stats)}", flush=True)
    for g in gs:
        g.close()


if __name__ == "__main__":
    main()
