"""bench.py --dump-outputs and the plain / --full split: a plain run times its steps and prints the contract
fields only, and writes what its last timed step computed (the wave's invalidated handles, the node
table's state flags) so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

SCALE = 14
FULL_ONLY = ("roofline", "rccl", "pipelined", "e2e", "configs2_single_gpu", "cpu_baseline")


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_small_graph_is_written_whole(tmp_path):
    ids = np.array([9, 2, 5], np.uint32)
    flags = np.arange(16, dtype=np.uint32)
    bench.dump_outputs(str(tmp_path), ids, 16, [3, 3, 7, 2], flags)
    d = _load(tmp_path)
    assert sorted(d) == ["counts", "invalidated_ids", "sample_handles", "state_flags"]
    assert d["invalidated_ids"].dtype == np.float64 and d["invalidated_ids"].tolist() == [2, 5, 9]
    assert d["sample_handles"].tolist() == list(range(16))
    assert d["state_flags"].dtype == np.float32 and d["state_flags"].tolist() == list(range(16))
    assert d["counts"].dtype == np.float64 and d["counts"].tolist() == [3, 3, 7, 2]


def test_dump_large_graph_is_a_fixed_sample(tmp_path):
    """Above DUMP_SAMPLE handles the same seeded handles are kept in every run: the ids written are
    exactly the invalidated ones among them, and the files stay far below 64 MB."""
    n = 3 * bench.DUMP_SAMPLE + 5
    ids = np.arange(1, n, 3, dtype=np.uint32)[::-1]   # handles 1, 4, 7, ... in descending order
    flags = (np.arange(n, dtype=np.uint32) % 3 == 1).astype(np.uint32) * 2
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), ids, n, [len(ids)] * 4, flags)
    bench.dump_outputs(str(b), ids.copy(), n, [len(ids)] * 4, flags)
    da, db = _load(a), _load(b)
    for k in da:
        assert np.array_equal(da[k], db[k])
    s = da["sample_handles"]
    # DUMP_SAMPLE draws with repeats from 3 x DUMP_SAMPLE handles leave 3 (1 - exp(-1/3)) = 0.85 of them distinct
    assert 0.8 * bench.DUMP_SAMPLE < len(s) <= bench.DUMP_SAMPLE and np.all(np.diff(s) > 0) and s[-1] < n
    assert np.array_equal(da["invalidated_ids"], s[s % 3 == 1])
    assert np.array_equal(da["state_flags"], (s % 3 == 1) * 2)
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) < 48 << 20


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_wave(pkg, gpu_available, tmp_path):
    """One plain run at R-MAT 14: the line has the contract fields and none of --full's legs; the dumped
    ids and state flags are those of the same wave run here on the same graph and roots."""
    from stl_fusion_amd import workloads as W
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--scale", str(SCALE), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=100, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    d = json.loads(line[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "invalidated nodes/s" and d["higher_is_better"] is True and d["dtype"] == "u64"
    assert not [k for k in FULL_ONLY if k in d]
    cfg = dict(W.CONFIGS["rmat24"])
    cfg["scale"] = SCALE
    n = W.n_slots(cfg)
    g = pkg.Graph(n)
    W.build(g, cfg)
    ws = pkg.WaveStats()
    ids = g.invalidate(W.roots_for(g, cfg), stats=ws)
    flags = g.dump_states()[1]
    g.close()
    out = _load(tmp_path / "out")
    assert np.array_equal(out["invalidated_ids"], np.sort(ids).astype(np.float64))
    assert np.array_equal(out["state_flags"], flags.astype(np.float32))
    assert out["counts"].tolist() == [len(ids), ws.v_inv, ws.e_trav, ws.levels]
    assert d["v_inv_per_step"] == len(ids)
