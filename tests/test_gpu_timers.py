"""The delay timers in device memory (fgi_timers_*, C-ABI 0.11) against the model of test_timers_model.py.

Every scenario there is driven on the engine and on the CPU oracle + model together; after every step the
engine must equal the model in the returned id set, fgi_dump_states over every handle, fgi_timers_list, the
fired count, fgi_timers_next_due and the statistics (armed == fired + dropped + stored). The gates at the end
check what the model does not cover: the status codes, fgi_restore, partitions, host_syncs and the fan-out."""
import ctypes as C

import numpy as np
import pytest

import fgo as O
from harness import CONSISTENT, F_DS, F_HD
from test_gpu_flagged import N as MIXED_N, N_DET as MIXED_DET, _engine, _mixed
from test_gpu_part_mutations import _group
import test_timers_model as M

pytestmark = pytest.mark.gpu


def _maker(pkg, labels=-1):
    def make(arrays, n_det, **kw):
        g = _engine(pkg, len(arrays[0]), *arrays, labels=labels, n_detached=n_det)
        return M.Driver(arrays, n_det, engine=g, fgi=pkg.fgi, **kw)
    return make


def test_chain(pkg, gpu_available):
    drv = M.scn_chain(_maker(pkg))
    assert drv.g.timers_stats()["runs"] == 1


@pytest.mark.parametrize("labels", [-1, 1])
def test_mixed_states(pkg, gpu_available, labels):
    drv = M.scn_mixed(_maker(pkg, labels))
    assert drv.c["fired"] >= 50 and drv.seen["overwrites"] >= 1 and drv.seen["stale"] >= 1


def test_word_and_tile_edges(pkg, gpu_available):
    M.scn_edges(_maker(pkg))


def test_slot_reuse(pkg, gpu_available):
    M.scn_slot_reuse(_maker(pkg))


@pytest.mark.parametrize("labels", [-1, 1])
def test_displacement(pkg, gpu_available, labels):
    M.scn_displacement(_maker(pkg, labels))


def test_cascading_timers(pkg, gpu_available):
    M.scn_cascading(_maker(pkg))


def test_batch(pkg, gpu_available):
    M.scn_batch(_maker(pkg))


def test_async_pair(pkg, gpu_available):
    M.scn_async(_maker(pkg))


def test_begin_reaches_own_slots(pkg, gpu_available):
    M.scn_begin_reaches_own_slots(_maker(pkg))


@pytest.mark.parametrize("labels", [-1, 1])
def test_displaced_and_reached(pkg, gpu_available, labels):
    """A displaced delayed node that the same call's cascade reached along an edge is armed under its detached
    handle, not under its slot and then moved (fgi_timer_stats.moved stays 0)."""
    M.scn_displaced_and_reached(_maker(pkg, labels))


def test_open_on_a_populated_graph(pkg, gpu_available):
    M.scn_open_populated(_maker(pkg))


def _runs_match(drv):
    assert drv.g.timers_stats()["runs"] == drv.c["runs"]


@pytest.mark.parametrize("labels", [-1, 1])
def test_past_one_grid(pkg, gpu_available, labels):
    """Every grid-stride loop of timers.hip on its second trip (test_past_one_grid_model states the sizes)."""
    drv = M.scn_past_one_grid(_maker(pkg, labels))
    _runs_match(drv)
    assert drv.c["runs"] == 5 and drv.seen["stale"] == 3000


def test_past_one_grid_capacity(pkg, gpu_available):
    """fgi_timers_run_due with a short id buffer at the large size: the scenario's first steps on an engine
    alone, then its tick(2) through the raw call. What it must return is taken from the scenario's plan
    (test_past_one_grid_model checks that against the model)."""
    fgi = pkg.fgi
    arrays, _, _, _, leaves, delays, one = M._grid_plan()
    want = M.grid_tick2_ids()
    g = _engine(pkg, len(arrays[0]), *arrays, n_detached=M.GRID_DET)
    g.timers_open(default_delay=7)
    g.timers_set_delay(leaves, delays)
    g.invalidate([0])
    g.invalidate([1])
    ids, fired = g.timers_run_due(1)
    assert list(ids) == [one] and fired == 1
    ids, n, fired = np.zeros(4096, np.uint32), C.c_uint64(), C.c_uint64()
    st = g.lib.fgi_timers_run_due(g.h, 2, ids.ctypes.data_as(C.POINTER(C.c_uint32)), len(ids), C.byref(n), C.byref(fired), None)
    assert st == fgi.ECAPACITY and n.value == len(want) == 5642 and fired.value == 5642
    assert np.array_equal(g.last_wave_ids(), want)
    assert g.timers_stats()["runs"] == 2 and g.timers_next_due() == (4, 278_491 - 1 - 5642)


def test_pool_growth(pkg, gpu_available):
    drv = M.scn_pool_growth(_maker(pkg))
    _runs_match(drv)
    assert drv.c["moved"] == 450 and drv.c["dropped"] == 150 and drv.c["fired"] == 3750


def test_delay_churn(pkg, gpu_available):
    """Entries that outlive their handle's delay code count towards the pool's capacity (timers.hip,
    tm_reserve): with a bound of the most codes there ever were, the second wave overflows the pool and every
    later call returns FGI_ESTATE."""
    drv = M.scn_delay_churn(_maker(pkg))
    _runs_match(drv)
    assert drv.c == dict(armed=4000, fired=4000, dropped=0, moved=0, runs=2)


def test_saturation(pkg, gpu_available):
    drv = M.scn_saturation(_maker(pkg))
    _runs_match(drv)
    assert drv.g.timers_next_due() == (pkg.fgi.TIMER_NONE, 0)


def test_batches_hand_out_each_detached_handle_once(pkg, gpu_available):
    """Two batches whose BEGIN_COMPUTE steps displace fewer live nodes than they have items (1 of 6, then 2 of
    6): nothing is released, so the three detached handles differ and the first still names its node. (A timer
    entry follows its node to such a handle; a handle given out twice would carry another node's entry.)"""
    n, n_det = 16, 8
    versions = O.version_of(21, np.arange(n, dtype=np.uint64)).copy()
    flags = np.full(n, 2, np.uint32)       # Invalidated: displaced without a detached handle
    flags[[0, 6, 7]] = 0                   # Computing: lives on under a detached handle
    none = np.zeros(0, np.uint32)
    g = _engine(pkg, n, versions, flags, none, none, np.zeros(0, np.uint64), n_detached=n_det)
    first, second = np.arange(0, 6, dtype=np.uint32), np.arange(6, 12, dtype=np.uint32)
    _, outs = g.run_batch([("begin_compute", first, versions[first] + np.uint64(2))])
    d1 = outs[0][outs[0] != pkg.fgi.NONE]
    assert len(d1) == 1 and outs[0][0] == d1[0]
    _, outs = g.run_batch([("begin_compute", second, versions[second] + np.uint64(2))])
    d2 = outs[0][outs[0] != pkg.fgi.NONE]
    assert len(d2) == 2
    assert len({int(d1[0]), int(d2[0]), int(d2[1])}) == 3, (d1, d2)
    v, f = g.get_state(np.concatenate([d1, d2]))
    assert list(v) == [versions[0], versions[6], versions[7]] and np.all((f & 3) == 0)


# ---- gates ---------------------------------------------------------------------------------------------------

def _chain_engine(pkg, n_det=0):
    arrays = M.chain_arrays(5, [(0, 1), (1, 2), (2, 3), (3, 4)], delayed=[3])
    return _engine(pkg, 5, *arrays, n_detached=n_det), arrays


def test_calls_before_open(pkg, gpu_available):
    fgi = pkg.fgi
    g, _ = _chain_engine(pkg)
    assert g.timers_stats() == dict(stored=0, armed=0, fired=0, dropped=0, moved=0, runs=0, last_kernel_ms=0.0)
    for call in (lambda: g.timers_set_delay([3], [5]), lambda: g.timers_set_now(1), lambda: g.timers_run_due(1),
                 g.timers_next_due, g.timers_list, g.timers_close):
        with pytest.raises(pkg.FgiError) as e:
            call()
        assert e.value.status == fgi.ESTATE
    g.invalidate([0])   # nothing is armed while the timers are closed
    g.timers_open(default_delay=5)
    assert g.timers_stats()["stored"] == 1   # ... and open finds the started node
    with pytest.raises(pkg.FgiError) as e:
        g.timers_open()
    assert e.value.status == fgi.ESTATE
    g.timers_close()
    assert g.timers_stats()["armed"] == 0


def test_clock_and_capacity(pkg, gpu_available):
    fgi = pkg.fgi
    g, _ = _chain_engine(pkg)
    g.timers_open(default_delay=5, now=10)
    g.invalidate([0])
    for call in (lambda: g.timers_set_now(9), lambda: g.timers_run_due(9)):
        with pytest.raises(pkg.FgiError) as e:
            call()
        assert e.value.status == fgi.EINVAL
    assert g.timers_next_due() == (15, 1) and g.timers_stats()["fired"] == 0
    with pytest.raises(pkg.FgiError) as e:
        g.timers_set_delay([5], [1])
    assert e.value.status == fgi.EINVAL
    ids, n, fired = np.zeros(1, np.uint32), C.c_uint64(), C.c_uint64()
    st = g.lib.fgi_timers_run_due(g.h, 15, ids.ctypes.data_as(C.POINTER(C.c_uint32)), 1, C.byref(n), C.byref(fired), None)
    assert st == fgi.ECAPACITY and n.value == 2 and fired.value == 1
    assert list(g.last_wave_ids()) == [3, 4]
    assert g.timers_next_due() == (fgi.TIMER_NONE, 0)
    st = g.lib.fgi_timers_run_due(g.h, 16, None, 0, C.byref(n), None, None)   # nothing due: no ids, no wave
    assert st == fgi.OK and n.value == 0 and g.timers_stats()["runs"] == 1
    assert list(g.last_wave_ids()) == [3, 4]


def test_restore_drops_every_entry(pkg, gpu_available):
    g, _ = _chain_engine(pkg)
    g.timers_open(now=3)
    g.timers_set_delay([3], [5])
    g.snapshot()
    g.invalidate([0])
    assert g.timers_stats()["stored"] == 1
    g.restore()
    st = g.timers_stats()
    assert st["stored"] == 0 and st["dropped"] == 1 and st["armed"] == 1
    assert len(g.timers_list()[0]) == 0
    g.invalidate([0])   # the clock and the delay stayed
    assert [list(a) for a in g.timers_list()[::2]] == [[3], [8]]


def test_partition_rank_is_refused(pkg, gpu_available):
    gs, _ = _group(pkg, 2, 64)
    for g in gs:
        with pytest.raises(pkg.FgiError) as e:
            g.timers_open()
        assert e.value.status == pkg.fgi.ENOTSUP


@pytest.mark.parametrize("labels", [-1, 1])
def test_host_syncs_are_the_twin_graphs(pkg, gpu_available, labels):
    """The same waves on twin graphs, timers open on one: same ids, same flagged sets, same statistics."""
    arrays, waves, _ = _mixed()
    a = _engine(pkg, MIXED_N, *arrays, labels=labels)
    b = _engine(pkg, MIXED_N, *arrays, labels=labels)
    a.timers_open(default_delay=4)
    for roots, imm, _, _, _, _ in waves:
        sa, sb = pkg.WaveStats(), pkg.WaveStats()
        ia, ib = a.invalidate(roots, imm, stats=sa), b.invalidate(roots, imm, stats=sb)
        assert np.array_equal(ia, ib)
        fa, fb = a.last_wave_flagged(), b.last_wave_flagged()
        assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1])
        for k in ("host_syncs", "levels", "v_inv", "e_trav", "e_match", "n_flagged", "roots", "f_total"):
            assert getattr(sa, k) == getattr(sb, k), k
    assert a.timers_stats()["stored"] > 20


def test_fanout_follows_a_timer_wave(pkg, gpu_available):
    g, _ = _chain_engine(pkg)
    g.timers_open(default_delay=5)
    assert list(g.subscribe([3, 4, 2], [0, 1, 1], [30, 40, 20])) == [0, 0, 0]
    g.invalidate([0])
    off, calls, hnd = g.last_wave_fanout(2)
    assert list(off) == [0, 0, 1] and list(calls) == [20] and list(hnd) == [2]
    ids, fired = g.timers_run_due(5)
    assert list(ids) == [3, 4] and fired == 1
    off, calls, hnd = g.last_wave_fanout(2)
    assert list(off) == [0, 1, 2] and list(calls) == [30, 40] and list(hnd) == [3, 4]
