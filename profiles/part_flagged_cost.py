"""The cost of the flagged-set post-pass per rank of a partition (fgi_part_last_flagged): an
in-process P-rank group on one GPU over an R-MAT graph with about 1% of its nodes delayed, K times restore +
one fgi_part_local_invalidate of 1,024 roots + every rank's accessor. Meant to run under
`rocprofv3 --kernel-trace --stats`, whose per-kernel table gives k_flag_list_part next to the wave's kernels;
on its own it prints the records per rank and the accessor's wall time.
Usage: python profiles/part_flagged_cost.py [scale] [P] [K] [edge factor, default 16]"""
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
from stl_fusion_amd.workloads import pick_roots  # noqa: E402

CONSISTENT, F_HD = 1, 16


def main():
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    P = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    K = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    ef = int(sys.argv[4]) if len(sys.argv) > 4 else 16
    seed = 0x5EED0027
    n = 1 << scale
    rng = np.random.default_rng(20)
    versions = O.version_of(seed, np.arange(n, dtype=np.uint64)).copy()
    flags = np.full(n, CONSISTENT, np.uint32)
    flags[rng.random(n) < 0.01] |= F_HD
    s, d = O.gen_rmat(scale, ef, seed)
    tags = versions[d]
    block = -(-n // P)
    gs = [pkg.Graph(block, rank=r, world=P) for r in range(P)]
    pkg.fgi.part_init_local(gs, n)
    slots = np.arange(n, dtype=np.uint32)
    for g in gs:
        g.part_register_nodes(slots, versions, flags)
        g.part_load_edges(s, d, tags)
        g.snapshot()
    roots = pick_roots(1024, n, 0x5EED1027, np.ones(n, np.uint8))
    acc, st, recs = [], None, None
    for k in range(K + 3):
        for g in gs:
            g.restore()
        st = pkg.fgi.part_local_invalidate(gs, roots)
        t0 = time.perf_counter()
        recs = [len(g.part_last_flagged()[1]) for g in gs]
        if k >= 3:
            acc.append((time.perf_counter() - t0) / P)
    acc = np.array(acc) * 1e3
    print(f"scale={scale} ef={ef} P={P} delayed={int((flags & F_HD != 0).sum())} v_inv={sum(x.v_inv for x in st)} "
          f"levels={st[0].levels} host_syncs={[x.host_syncs for x in st]} kernel_ms={[round(x.kernel_ms, 4) for x in st]} "
          f"records_per_rank={recs} accessor_ms_per_rank median={np.median(acc):.4f} min={acc.min():.4f}")


if __name__ == "__main__":
    main()
