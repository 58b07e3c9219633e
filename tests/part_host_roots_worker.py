"""One rank of the multi-process host-roots test (tests/test_gpu_part_host_roots.py): the partitioned engine
in a process of its own (fgi_part_init_host: every collective an all-gather through torch.distributed over
gloo), all ranks on GPU 0, driven the way a multi-GPU host drives a scope flush: the roots are numpy arrays
in host memory (fgi_part_invalidate_host / fgi_part_invalidate_bits), the ids and the bitmap come back in
the host's numbering. No device tensor appears here. Launched by torch.distributed.run; writes this rank's
results to <out>/rank<r>.npz for the parent to compare with the oracle (the oracle is used here only to pick
the roots the parent's oracle run uses)."""
import argparse
import ctypes
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

# the scenario of part_host_worker.py (shared with the parent test)
RMAT = dict(scale=13, ef=8, seed=0x5EED0027, sseed=0x5EED00C0)
WAVES = [(48, 0x5EED1027), (16, 99), (48, 0x5EED1027)]


def _d2h(ptr, n):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.zeros(n, np.uint32)
    if n:
        assert hip.hipMemcpy(out.ctypes.data, ctypes.c_void_p(ptr), 4 * n, 2) == 0   # hipMemcpyDeviceToHost
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--labels", type=int, default=0)
    args = ap.parse_args()

    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=60))   # a lost peer ends every collective
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    import _pkg
    import fgo as O
    pkg = _pkg.load()
    n = 1 << RMAT["scale"]
    block = -(-n // world)
    g = pkg.Graph(block, rank=rank, world=world, labels=args.labels)
    g.part_init_host(n)
    g.part_synth_rmat(RMAT["scale"], RMAT["ef"], RMAT["seed"], 0, RMAT["sseed"])
    s, _ = O.gen_rmat(RMAT["scale"], RMAT["ef"], RMAT["seed"])
    deg = np.bincount(s, minlength=n)
    res = {}
    for w, (k, rseed) in enumerate(WAVES):
        roots = O.gen_roots(k, n, rseed, deg)
        imm = (np.arange(len(roots)) % 5 == 0).astype(np.uint8)
        # the three ways to ask: ids with the call, the bitmap with the call, the count alone
        if w == 0:
            res[f"w{w}_call"] = g.part_invalidate_host(roots, imm)
        elif w == 1:
            bits, _ = g.part_invalidate_host(roots, imm, want="bits")
            res[f"w{w}_call"] = (pkg.fgi.bits_to_ids(bits) + rank * block).astype(np.uint32)
        else:
            g.part_invalidate_host(roots, imm, want=None)
            res[f"w{w}_call"] = g.part_last_wave_ids()
        res[f"w{w}_ids"] = g.part_last_wave_ids()
        bits, nv = g.part_last_wave_bits()
        res[f"w{w}_bits"], res[f"w{w}_n"] = bits, np.array([nv], np.uint64)
        ptr, nd = g.part_wave_ids_dev()
        res[f"w{w}_dev"] = _d2h(ptr, nd)
        res[f"w{w}_export"] = g.part_export_ids()
    res["block"] = np.array([block, n, world], np.uint64)
    np.savez(os.path.join(args.out, f"rank{rank}.npz"), **res)
    g.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
