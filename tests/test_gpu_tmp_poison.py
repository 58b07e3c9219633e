"""FGI_TMP_POISON=1 (read at fgi_create): every device temporary (Tmp) is handed out filled with 0xA5 bytes,
fresh or from the graph's cache. A fresh hipMalloc is often zero and a cached block never is, so a buffer
that is read before it is fully written or memset passes on the first and fails on the second. The loads,
the synthetic generators and the staged host roots all take their call-lifetime memory through Tmp: the
existing small scenarios run again under the switch, their oracle comparisons unchanged."""
import json
import os

import numpy as np
import pytest

import fgo as O
import test_gpu_labels as labels_tests        # (modules, not their test functions: those would be collected here too)
import test_gpu_part_load as load_tests
import test_gpu_part_shard as shard_tests
from test_gpu_flagged import _engine
from test_gpu_part_state_view import _build_with

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "mixed_states_imm.json")


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("FGI_TMP_POISON", "1")   # before any graph of the test is created


def test_poisoned_partition_codes(pkg, gpu_available):
    """part_codes_choose, part_rebuild_lists, part_store_in and fgi_part_register_nodes."""
    load_tests.test_partition_codes_mixed_state_graph(pkg, gpu_available, P=3, direction=2, tpb=0)


def test_poisoned_partition_loads(pkg, gpu_available):
    load_tests.test_partition_loads_mixed_state_graph(pkg, gpu_available, P=2, direction=1, labels=0)


def test_poisoned_shard_loads(pkg, gpu_available):
    shard_tests.test_shards_load_mixed_state_graph(pkg, gpu_available, P=3, direction=2, labels=1, tpb=0,
                                                   order="shard_then_replicated")


def test_poisoned_labelled_rmat(pkg, gpu_available):
    """labels_choose and the single device's generator."""
    labels_tests.test_labelled_rmat_waves_match_oracle(pkg, gpu_available, stale=50, direction=0)


def test_poisoned_part_synth_rmat(pkg, gpu_available):
    """fgi_part_synth_rmat with partition codes: one wave of two in-process ranks against the single engine."""
    scale, ef, seed, sseed, stale, P = 10, 8, 0x5EED0027, 0x5EED00C0, 50, 2
    n = 1 << scale
    block = n // P
    one = pkg.Graph(n, labels=-1)
    one.synth_rmat(scale, ef, seed, stale, sseed)
    deg, _ = one.degrees()
    roots = O.gen_roots(32, n, 0x5EED1027, deg[:n])
    ws = pkg.WaveStats()
    want = np.sort(one.invalidate(roots, stats=ws))
    v1, f1 = one.dump_states()
    one.close()
    assert len(want) > len(roots)   # the wave spreads
    gs = [pkg.Graph(block, rank=r, world=P, labels=1) for r in range(P)]
    pkg.fgi.part_init_local(gs, n)
    for g in gs:
        g.part_synth_rmat(scale, ef, seed, stale, sseed)
    stats = pkg.fgi.part_local_invalidate(gs, roots)
    ids = np.sort(np.concatenate([g.part_export_ids() for g in gs]))
    assert np.array_equal(ids, want), (len(ids), len(want))
    assert sum(x.v_inv for x in stats) == ws.v_inv and sum(x.e_trav for x in stats) == ws.e_trav
    for r, g in enumerate(gs):
        v, f = g.dump_states()
        lo, hi = r * block, (r + 1) * block
        assert np.array_equal(v[:hi - lo], v1[lo:hi]) and np.array_equal(f[:hi - lo], f1[lo:hi]), r
        g.close()


def test_poisoned_host_root_stages(pkg, gpu_available):
    """The shared root stage on a golden fixture: one fgi_invalidate_async_host wave, one
    fgi_part_invalidate_host wave (a partition of one rank), each against the fixture's invalidated set."""
    doc = json.load(open(GOLDEN))
    n = doc["n_slots"]
    arrays = (np.array(doc["versions"], np.uint64), np.array(doc["state_flags"], np.uint32),
              np.array(doc["used"], np.uint32), np.array(doc["dependant"], np.uint32), np.array(doc["tags"], np.uint64))
    roots = np.array(doc["roots"], np.uint32)
    imm = np.array(doc["immediately"], np.uint8)
    want = np.array(doc["expected"]["inv"], np.uint32)
    assert imm.any() and len(want) > len(roots)
    g = _engine(pkg, n, *arrays)
    assert np.array_equal(g.wave_wait_ids(g.invalidate_async_host(roots, imm)), want)
    g.close()
    gs, _ = _build_with(pkg, 1, n, *arrays, options={}, labels=1)
    assert np.array_equal(gs[0].part_invalidate_host(roots, imm), want)
    gs[0].close()
