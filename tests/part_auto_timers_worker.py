"""One rank of the multi-process auto-invalidation timer test (tests/test_gpu_part_auto_timers.py): the partitioned
engine in a process of its own (fgi_part_init_host: every collective an all-gather through torch.distributed over
gloo), all ranks on GPU 0. The rank makes test_part_auto_timers_model.py's ProcPlan calls through the Graph methods
(part_timers_auto_open, part_timers_set_auto_delay, part_begin_compute, part_set_output with transient flags,
part_timers_run_due); after every step it records its entries with their kinds, its counters and its states.
Started once per rank with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set; writes <out>/rank<r>.npz for the
parent to compare with the model."""
import argparse
import datetime
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


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
    from test_part_auto_timers_model import ProcPlan as W
    pkg = _pkg.load()
    n = W.N
    block = -(-n // world)
    g = pkg.Graph(block, n_detached=W.N_DET, rank=rank, world=world)
    g.part_init_host(n)
    res = {}

    def snap(k, ids=None, counts=None):
        res[f"s{k}_h"], res[f"s{k}_v"], res[f"s{k}_d"], res[f"s{k}_k"] = g.part_timers_list_ex()
        res[f"s{k}_sv"], res[f"s{k}_sf"] = g.dump_states()
        st, au = g.timers_stats(), g.part_timers_auto_stats()
        res[f"s{k}_stats"] = np.array([st[x] for x in ("armed", "fired", "dropped", "moved")], np.uint64)
        res[f"s{k}_auto"] = np.array([au[x] for x in ("armed_auto", "merged", "fired_auto")], np.uint64)
        if ids is not None:
            res[f"s{k}_ids"] = ids
        if counts is not None:
            res[f"s{k}_fired"] = np.array(counts, np.uint64)
            res[f"s{k}_fdet"] = g.part_timers_fired_detached()

    g.part_timers_open()
    g.part_timers_auto_open(W.DEFAULTS["default_auto"], W.DEFAULTS["default_transient"])
    g.part_timers_set_auto_delay(W.SLOTS, W.AUTO_DELAYS, W.TRANS_DELAYS)
    g.part_timers_set_delay(W.DELAYED, [W.DELAY] * len(W.DELAYED))
    g.part_begin_compute(W.SLOTS, W.VERSIONS, W.HAS_DELAY)
    g.part_set_output(W.SLOTS, transient=W.TRANSIENT)
    snap(0)
    ids, fired, det = g.part_timers_run_due(W.TICKS[0])
    snap(1, ids, (fired, det))
    g.timers_set_now(W.MOVE_AT)
    res["moved"], _ = g.part_begin_compute(W.MOVED, W.MOVED_VERSIONS)
    snap(2)
    for k, now in ((3, W.TICKS[1]), (4, W.TICKS[2])):
        ids, fired, det = g.part_timers_run_due(now)
        snap(k, ids, (fired, det))
    np.savez(os.path.join(args.out, f"rank{rank}.npz"), **res)
    g.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
