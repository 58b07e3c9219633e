"""Seeded random operation walks (walk_model.py) on the engine with the delay timers, the auto timers, the replica
fan-out and the state view open on one single-device graph, against the combined model `FullDriver`; the same walk
with the layers opened late; on an engine pair of which one opens nothing; and the timers' share of it on a
partition against `PartDriver`.

After every driver call the engine must equal the model in the returned ids, fgi_dump_states over every handle,
fgi_timers_list / _list_ex, the timers' and auto statistics, fgi_timers_next_due, the fan-out of the call's cascades,
fgi_sub_stats and the six planes of the state view. test_walk_model.py checks, without a GPU, that these walks reach
the rules they are for and that a model with a neighbouring rule ends elsewhere. A failure names the seed, the step
and the operation; `walk(..., stop_at=k)` replays a prefix."""
import numpy as np
import pytest

from test_gpu_flagged import _engine
import test_gpu_part_timers as PT
import walk_model as W
from walk_model import SEEDS, FullDriver

pytestmark = pytest.mark.gpu

_alone = {}


def _model_alone(seed, **kw):
    """The seed's walk on the model alone: the counters the engine's walk must end with."""
    key = (seed, tuple(sorted(kw.items())))
    if key not in _alone:
        _alone[key] = W.counters(W.full_walk(FullDriver, seed, **{k: dict(v) if k == "layers" else v for k, v in kw.items()})[0])
    return _alone[key]


def _maker(pkg, labels=-1):
    def make(arrays, n_det, **kw):
        g = _engine(pkg, len(arrays[0]), *arrays, labels=labels, n_detached=n_det)
        return FullDriver(arrays, n_det, engine=g, fgi=pkg.fgi, **kw)
    return make


@pytest.mark.parametrize("labels", [-1, 1])
@pytest.mark.parametrize("seed", SEEDS)
def test_walk_everything_open(pkg, gpu_available, seed, labels):
    """1,000 slots + 90 detached handles (1,090: every per-handle kernel ends in a partial wavefront and a partial
    bitmap word), 6,000 edges, every layer open from the start, 200 operations."""
    assert (W.N + W.N_DET) % 64 != 0
    drv, log, _ = W.full_walk(_maker(pkg, labels), seed)
    assert drv.view is not None and drv.auto and drv.timers_on
    assert W.counters(drv) == _model_alone(seed)
    st = drv.g.view_stats()
    assert st.full_builds == 1 and st.updates >= drv.c["runs"]   # every fired tick's wave reached the view
    drv.g.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_walk_features_opened_late(pkg, gpu_available, seed):
    """fgi_timers_open, fgi_timers_auto_open, the first fgi_subscribe and fgi_state_view_open each at a random step
    of the first half, on a graph that already holds detached nodes, stale rows and a last wave."""
    layers = W.late_layers(seed)
    drv, log, _ = W.full_walk(_maker(pkg), seed, layers=layers)
    assert W.counters(drv) == _model_alone(seed, layers=tuple(sorted(layers.items())))
    drv.g.close()


# ---- an engine pair ----------------------------------------------------------------------------------------
STAT_FIELDS = ("levels", "v_inv", "e_trav", "e_match", "n_flagged", "host_syncs")


class Pair:
    """Graph-like: every call that changes or reads the graph goes to `a` (the layers are its alone) and to `b`
    (which opens none); what the two return must be equal: ids, the statistics' counts, flagged sets, states."""

    def __init__(self, pkg, a, b):
        self.pkg, self.a, self.b = pkg, a, b
        self.tickets = {}
        self.fire = np.zeros(0, np.uint32)
        self.compared = 0

    def __getattr__(self, name):           # the layers' own calls: timers_*, subscribe, fan-out, the view, ...
        return getattr(self.a, name)

    def close(self):
        self.a.close()
        self.b.close()

    def _same(self, what, ia, ib, sa, sb, fa, fb, fields=STAT_FIELDS):
        assert np.array_equal(ia, ib), f"{what}: ids differ ({len(ia)} vs {len(ib)})"
        for k in fields:
            assert getattr(sa, k) == getattr(sb, k), f"{what}: {k} {getattr(sa, k)} vs {getattr(sb, k)}"
        assert len(fa) == len(fb) and all(np.array_equal(x, y) for x, y in zip(fa, fb)), f"{what}: flagged sets differ"
        self.compared += 1

    def set_option(self, opt, value):
        self.a.set_option(opt, value)
        self.b.set_option(opt, value)

    def invalidate(self, roots, imm=None):
        sa, sb = self.pkg.WaveStats(), self.pkg.WaveStats()
        ia, ib = self.a.invalidate(roots, imm, stats=sa), self.b.invalidate(roots, imm, stats=sb)
        self._same("invalidate", ia, ib, sa, sb, self.a.last_wave_flagged(), self.b.last_wave_flagged())
        return ia

    def invalidate_async_host(self, roots, imm=None):
        t = self.a.invalidate_async_host(roots, imm)
        self.tickets[t] = self.b.invalidate_async_host(roots, imm)
        return t

    def wave_wait_ids(self, t):
        sa, sb = self.pkg.WaveStats(), self.pkg.WaveStats()
        ia, ib = self.a.wave_wait_ids(t, stats=sa), self.b.wave_wait_ids(self.tickets[t], stats=sb)
        self._same("ticket", ia, ib, sa, sb, self.a.wave_wait_flagged(t), self.b.wave_wait_flagged(self.tickets[t]))
        return ia

    def begin_compute(self, slots, versions, has_delay=None):
        sa, sb = self.pkg.WaveStats(), self.pkg.WaveStats()
        oa = self.a.begin_compute(slots, versions, has_delay, stats=sa)
        ob = self.b.begin_compute(slots, versions, has_delay, stats=sb)
        assert np.array_equal(oa, ob), "begin_compute: detached handles differ"
        self._same("begin_compute", self.a.last_wave_ids(), self.b.last_wave_ids(), sa, sb,
                   self.a.last_wave_flagged(), self.b.last_wave_flagged())
        return oa

    def add_used(self, dependants, used):
        ra, rb = self.a.add_used(dependants, used), self.b.add_used(dependants, used)
        assert np.array_equal(ra, rb), "add_used: results differ"
        return ra

    def set_output(self, handles, transient=None):
        sa, sb = self.pkg.WaveStats(), self.pkg.WaveStats()
        (oa, ia), (ob, ib) = (g.set_output(handles, stats=s, transient=transient) for g, s in ((self.a, sa), (self.b, sb)))
        assert np.array_equal(oa, ob), "set_output: out_set differs"
        self._same("set_output", ia, ib, sa, sb, self.a.last_wave_flagged(), self.b.last_wave_flagged())
        return oa, ia

    def run_batch(self, steps):
        sa, sb = self.pkg.fgi.BatchStats(), self.pkg.fgi.BatchStats()
        (ia, oa), (ib, ob) = self.a.run_batch(steps, stats=sa), self.b.run_batch(steps, stats=sb)
        for k, (x, y) in enumerate(zip(oa, ob)):
            assert (x is None and y is None) or np.array_equal(x, y), f"run_batch: step {k}'s out differs"
        self._same("run_batch", ia, ib, sa, sb, self.a.last_batch_flagged(), self.b.last_batch_flagged())
        return ia, oa

    def timers_run_due(self, now):
        """The tick on `a`; on `b` the model's fired handles as the roots of a wave with immediately = 1. The tick's
        roots are already on the device, fgi_invalidate uploads its own: host_syncs is not compared here."""
        sa, sb = self.pkg.WaveStats(), self.pkg.WaveStats()
        ia, fired = self.a.timers_run_due(now, stats=sa)
        if len(self.fire):
            ib = self.b.invalidate(self.fire, np.ones(len(self.fire), np.uint8), stats=sb)
            self._same("tick", ia, ib, sa, sb, self.a.last_wave_flagged(), self.b.last_wave_flagged(), STAT_FIELDS[:-1])
        return ia, fired

    def release(self, handles):
        self.a.release(handles)
        self.b.release(handles)

    def prune(self):
        self.b.prune()
        return self.a.prune()

    def prune_range(self, lo, count):
        self.b.prune_range(lo, count)
        return self.a.prune_range(lo, count)

    def dump_states(self):
        (va, fa), (vb, fb) = self.a.dump_states(), self.b.dump_states()
        assert np.array_equal(va, vb) and np.array_equal(fa, fb), "the pair's states differ"
        return va, fa


@pytest.mark.parametrize("seed", SEEDS)
def test_walk_twins(pkg, gpu_available, seed):
    """test_gpu_timers.py's test_host_syncs_are_the_twin_graphs over the whole operation mix: the walk on two engines,
    every layer open on one and none on the other. Every call returns the same ids, flagged sets and counts of
    levels, v_inv, e_trav, e_match, n_flagged and host_syncs, and the open one still equals the model."""
    def make(arrays, n_det, **kw):
        a, b = (_engine(pkg, len(arrays[0]), *arrays, n_detached=n_det) for _ in range(2))
        for g in (a, b):   # fgi.h: with the filter on, e_match depends on which lane reaches a node first
            g.set_option(pkg.fgi.OPT_DEAD_FILTER, 0)
        return FullDriver(arrays, n_det, engine=Pair(pkg, a, b), fgi=pkg.fgi, **kw)
    drv, log, _ = W.full_walk(make, seed)
    assert drv.g.compared >= 150
    assert W.counters(drv) == _model_alone(seed)
    st = drv.g.b.timers_stats()
    assert st["armed"] == 0 and st["runs"] == 0
    assert drv.g.b.sub_stats()["pool"] == 0 and drv.g.b.view_stats().full_builds == 0
    drv.g.close()


# ---- a partition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("P", [2, 3])
def test_walk_on_partitions(pkg, gpu_available, P, seed):
    """What PartDriver models of the walk (waves, begin_compute / add_used / set_output, batches, ticks, release) on
    512 slots over P in-process ranks (three ranks: ragged ranges), 100 operations. Group.tick compares
    fgi_part_timers_fired_detached wherever a detached entry comes due."""
    import test_part_timers_model as PM
    drv, log, _ = W.part_walk(PT._maker(pkg, P), seed)
    alone = W.part_walk(PM._alone(P), seed)[0]
    assert W.counters(drv) == W.counters(alone)
    assert drv.seen["det_fired"] == sum(len(d) for _, det in drv.ticks for d in det)
    drv.g.close()
