"""The sharded partition loads across real process boundaries: two or three processes (torch.distributed.run,
all on GPU 0, host collectives over gloo as in test_gpu_part_host.py) each register the nodes r::P and load the
edges r::P of an R-MAT scale-13, edge-factor-8 graph with 50% stale tags and partition codes on — nearly every
item sits on a rank that does not own it, and the variable-size all-gather and all-to-all of the two calls run
through the host transport. World size 3 is ragged. The parent checks the ids, V_inv, the first wave's E_trav
and the node words of the worker's three waves against the oracle on the whole graph. Most of a case's time is
process start-up."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import fgo as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import part_shard_worker as SW  # noqa: E402


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch(P, tmp_path):
    out = tmp_path / f"p{P}"
    out.mkdir()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={P}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(HERE, "part_shard_worker.py"), "--out", str(out)]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return [dict(np.load(out / f"rank{q}.npz")) for q in range(P)]


@pytest.mark.parametrize("P", [2, 3])
def test_sharded_loads_across_processes(gpu_available, tmp_path, P):
    ranks = _launch(P, tmp_path)
    c = SW.RMAT
    n = 1 << c["scale"]
    s, d = O.gen_rmat(c["scale"], c["ef"], c["seed"])
    o = O.Oracle(n)
    o.load_graph(O.version_of(c["seed"], np.arange(n)), None, s, d, O.gen_tags(s, d, c["seed"], c["stale"], c["sseed"]))
    deg = np.bincount(s, minlength=n)
    for w, (k, rseed) in enumerate(SW.WAVES):
        roots = O.gen_roots(k, n, rseed, deg)
        imm = (np.arange(len(roots)) % 5 == 0).astype(np.uint8)
        o.clear_log()
        st = o.invalidate_slots(roots, imm)
        ids = np.concatenate([r[f"w{w}_ids"] for r in ranks])
        assert np.array_equal(np.sort(ids), np.sort(o.inv_log())), f"wave {w}: {len(ids)} vs {st.v_inv}"
        assert sum(int(r[f"w{w}_stats"][0]) for r in ranks) == st.v_inv
        if w == 0:
            assert sum(int(r[f"w{w}_stats"][1]) for r in ranks) == st.e_trav
        ov, of = o.dump_states()
        for q, res in enumerate(ranks):
            block = int(res["block"][0])
            lo, hi = q * block, min(n, (q + 1) * block)
            assert np.array_equal(res[f"w{w}_ver"][:hi - lo], ov[lo:hi]), f"wave {w}: rank {q} versions differ"
            assert np.array_equal(res[f"w{w}_flags"][:hi - lo], of[lo:hi]), f"wave {w}: rank {q} flags differ"
    o.close()
