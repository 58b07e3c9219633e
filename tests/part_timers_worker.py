"""One rank of the multi-process delay-timer test (tests/test_gpu_part_timers.py): the partitioned engine in a
process of its own (fgi_part_init_host: every collective an all-gather through torch.distributed over gloo), all
ranks on GPU 0. The rank loads test_part_timers_model.py's edges graph, opens its timers and makes the scenario's
calls through the Graph methods (part_timers_open, part_timers_set_delay, part_invalidate_host,
part_timers_run_due, part_begin_compute); after every step it records its ids, its entries, its counts and its
states. Launched by torch.distributed.run; writes <out>/rank<r>.npz for the parent to compare with the model."""
import argparse
import datetime
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

TICKS = ((3, 2), (4, 3), (5, 4), (6, 50))   # (step, now) behind the displacement


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()

    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=60))   # a lost peer ends every collective
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    import _pkg
    import test_part_timers_model as PM
    pkg = _pkg.load()
    n = PM.EDGE_N
    (versions, flags, src, dst, tags), others, delays = PM.edge_plan(n, world)
    block = -(-n // world)
    g = pkg.Graph(block, n_detached=PM.EDGE_DET, rank=rank, world=world)
    g.part_init_host(n)
    present = np.nonzero(versions)[0].astype(np.uint32)
    g.part_register_nodes(present, versions[present], flags[present])
    g.part_load_edges(src, dst, tags)
    res = {}

    def snap(k, ids=None, counts=None):
        res[f"s{k}_h"], res[f"s{k}_v"], res[f"s{k}_d"] = g.timers_list()
        res[f"s{k}_sv"], res[f"s{k}_sf"] = g.dump_states()
        res[f"s{k}_runs"] = np.array([g.timers_stats()["runs"]], np.uint64)
        if ids is not None:
            res[f"s{k}_ids"] = ids
        if counts is not None:
            res[f"s{k}_fired"] = np.array(counts, np.uint64)
            res[f"s{k}_fdet"] = g.part_timers_fired_detached()

    g.part_timers_open()
    g.part_timers_set_delay(others, delays[others])
    snap(0, g.part_invalidate_host([PM.EDGE_HUB]))
    ids, fired, det = g.part_timers_run_due(1)
    snap(1, ids, (fired, det))
    moved = np.array(PM.EDGE_MOVED, np.uint32)
    res["moved"], _ = g.part_begin_compute(moved, versions[moved] + np.uint64(10))
    snap(2)
    for k, now in TICKS:
        ids, fired, det = g.part_timers_run_due(now)
        snap(k, ids, (fired, det))
    np.savez(os.path.join(args.out, f"rank{rank}.npz"), **res)
    g.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
