"""One rank of the multi-process sharded-load test (tests/test_gpu_part_shard_host.py): the partition joined
with host collectives (fgi_part_init_host over gloo), all ranks on GPU 0. Rank r registers nodes r::P and loads
edges r::P of the R-MAT graph below through fgi_part_register_shard / fgi_part_load_edges_shard (partition
codes on), runs part_host_worker's three waves and writes its results to <out>/rank<r>.npz for the parent."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from part_host_worker import WAVES  # noqa: E402

RMAT = dict(scale=13, ef=8, seed=0x5EED0027, sseed=0x5EED00C0, stale=50)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()

    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    import _pkg
    import fgo as O
    pkg = _pkg.load()
    n = 1 << RMAT["scale"]
    block = -(-n // world)
    g = pkg.Graph(block, rank=rank, world=world, labels=1)
    g.part_init_host(n)
    s, d = O.gen_rmat(RMAT["scale"], RMAT["ef"], RMAT["seed"])
    tags = O.gen_tags(s, d, RMAT["seed"], RMAT["stale"], RMAT["sseed"])
    slots = np.arange(n, dtype=np.uint32)[rank::world]
    g.part_register_shard(slots, O.version_of(RMAT["seed"], slots.astype(np.uint64)))
    g.part_load_edges_shard(s[rank::world], d[rank::world], tags[rank::world])
    deg = np.bincount(s, minlength=n)
    res = {}
    for w, (k, rseed) in enumerate(WAVES):
        roots = O.gen_roots(k, n, rseed, deg)
        imm = (np.arange(len(roots)) % 5 == 0).astype(np.uint8)
        d_roots = torch.from_numpy(roots.astype(np.int32)).cuda()
        d_imm = torch.from_numpy(imm).cuda()
        st = pkg.WaveStats()
        g.part_invalidate(len(roots), d_roots.data_ptr(), d_imm.data_ptr(), st)
        res[f"w{w}_ids"] = g.part_export_ids()
        res[f"w{w}_stats"] = np.array([st.v_inv, st.e_trav, st.levels, st.host_syncs, st.pull_levels], np.uint64)
        v, f = g.dump_states()
        res[f"w{w}_ver"], res[f"w{w}_flags"] = v, f
    res["block"] = np.array([block, n, world], np.uint64)
    np.savez(os.path.join(args.out, f"rank{rank}.npz"), **res)
    g.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
