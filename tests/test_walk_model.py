"""walk_model.py alone (no GPU), over the seeds and sizes test_gpu_walk.py uses: the walks are deterministic, they
reach every rule the issue lists (so the GPU cases cannot pass on nothing), few operations are replaced, and a model
with one neighbouring rule changed ends somewhere else (so an engine that built that rule would be caught)."""
import collections

import numpy as np
import pytest

import test_auto_timers_model as A
import test_part_timers_model as PM
import test_timers_model as M
import walk_model as W
from walk_model import FullDriver, SEEDS
from test_timers_model import NONE

_cache = {}


def _walked(seed, cls=FullDriver):
    """(driver, log, replaced) of the seed's walk on the model alone; computed once per class."""
    if (seed, cls) not in _cache:
        _cache[seed, cls] = W.full_walk(cls, seed)
    return _cache[seed, cls]


def test_full_driver_keeps_the_scenarios():
    """FullDriver restates AutoDriver's tick and batch with hooks: the hand-written scenarios pass on it unchanged."""
    make = lambda arrays, n_det, **kw: FullDriver(arrays, n_det, **kw)
    for scn in (A.scn_chain, A.scn_selection, A.scn_no_defaults, A.scn_ioso_delay, A.scn_merge, A.scn_delay_then_auto,
                A.scn_displacement, A.scn_batch, A.scn_cascading, A.scn_start_auto):
        scn(make)
    for scn in (M.scn_chain, M.scn_mixed, M.scn_slot_reuse, M.scn_displacement, M.scn_cascading, M.scn_batch,
                M.scn_saturation):
        scn(make)
    drv = A.scn_batch(make)
    assert drv.seen["resolved_detached"] == 2 and drv.seen["resolved_none"] == 2
    assert drv.ca == dict(armed_auto=4, merged=2, fired_auto=4)


@pytest.mark.parametrize("seed", SEEDS)
def test_same_seed_same_trace(seed):
    a = W.full_walk(FullDriver, seed)
    b = _walked(seed)
    assert a[1] == b[1] and a[2] == b[2]
    assert a[0].fingerprint() == b[0].fingerprint()
    short = W.full_walk(FullDriver, seed, stop_at=60)
    assert short[1] == b[1][:len(short[1])] and len({e[0] for e in short[1] if e[0] >= 0}) == 60


class HighestFirst(FullDriver):
    """Another numbering of the detached handles: the highest free one first."""
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.free.reverse()


@pytest.mark.parametrize("seed", SEEDS)
def test_walk_does_not_depend_on_detached_numbering(seed):
    """Which number a displaced node gets is the engine's choice. The walk lists detached handles in the order they
    were handed out, so another numbering walks through the same operations on the same nodes: the floors checked
    here hold for the walk the engine takes (test_gpu_walk.py asserts the same counters)."""
    a, b = _walked(seed), W.full_walk(HighestFirst, seed)
    assert [e[:3] for e in a[1]] == [e[:3] for e in b[1]]
    assert W.counters(a[0]) == W.counters(b[0])
    assert a[0].fingerprint() != b[0].fingerprint()      # ... under other handle numbers


@pytest.mark.parametrize("seed", SEEDS)
def test_walk_is_not_vacuous(seed):
    drv, log, _ = _walked(seed)
    c, s = drv.c, drv.seen
    assert c["moved"] >= 1 and drv.ca["merged"] >= 1 and c["runs"] >= 5, (c, drv.ca)
    for k in ("stale", "displaced_armed", "never", "fired_without_ds", "resolved_detached", "resolved_none"):
        assert s[k] >= 1, (k, s)
    assert all(drv.routes[r] >= 1 for r in W.ROUTES), drv.routes
    assert s["subs_moved"] >= 1 and s["subs_released"] >= 1 and s["sub_invalidated"] >= 1, s
    assert c["armed"] == c["fired"] + c["dropped"] + len(drv.entries), c
    assert drv.sc["delivered"] + drv.sc["dropped"] + drv.live == drv.sc["stored"], drv.sc
    ops = collections.Counter(e[1] for e in log)
    assert all(ops[o] >= 1 for o in W.ALL_OPS), ops
    # a tick that fired nothing after a wave stood (the "last wave's results stay" rule is exercised)
    assert sum(1 for t in drv.trace if t[0] == "tick" and t[2] == 0) >= 1


def test_walks_reach_the_rare_rules():
    drvs = [_walked(seed)[0] for seed in SEEDS]
    assert sum(d.seen["overwrites"] for d in drvs) >= 1
    assert sum(d.seen["reused_after_drop"] for d in drvs) >= 1


@pytest.mark.parametrize("seed", SEEDS)
def test_few_operations_are_replaced(seed):
    _, log, replaced = _walked(seed)
    assert replaced == sum(1 for e in log if e[2] is not None)
    assert replaced <= W.STEPS // 10, replaced
    assert len([e for e in log if e[0] >= 0 and not e[1].startswith("open:")]) == W.STEPS


@pytest.mark.parametrize("seed", SEEDS)
def test_late_layers_open_in_order(seed):
    """The late walk: every layer opens in the first half, timers before auto, the view last; the walk still fires
    timers and delivers subscriptions afterwards."""
    layers = W.late_layers(seed)
    order = [name for k in sorted(layers) for name in layers[k]]
    assert sorted(order) == sorted(W.LAYERS) and order[-1] == "view" and order.index("timers") < order.index("auto")
    assert max(layers) < W.STEPS // 2
    drv, log, _ = W.full_walk(FullDriver, seed, layers=layers)
    assert drv.c["runs"] >= 1 and drv.sc["delivered"] >= 1 and drv.ca["armed_auto"] >= 1
    # the graph the first layer opens on already holds a last wave and displaced nodes
    before = [e[1] for e in log if 0 <= e[0] < min(layers)]
    assert "wave" in before and ("compute" in before or "batch" in before), before


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("seed", SEEDS)
def test_partition_walk_is_not_vacuous(P, seed):
    drv, log, replaced = W.part_walk(PM._alone(P), seed)
    c, s = drv.c, drv.seen
    assert c["runs"] >= 3 and c["moved"] >= 1 and s["displaced_armed"] >= 1 and s["det_moved"] >= 1, (c, s)
    assert c["armed"] == c["fired"] + c["dropped"] + len(drv.entries)
    assert replaced <= W.PART_STEPS // 10
    assert set(e[1] for e in log if e[0] >= 0) <= set(W.PART_OPS)
    assert W.PART_N % P != 0 or P == 2         # three ranks: ragged ranges


def test_partition_walks_fire_a_detached_entry():
    assert sum(W.part_walk(PM._alone(P), seed)[0].seen["det_fired"] for P in (2, 3) for seed in SEEDS) >= 1


# ---- rule sensitivity: one neighbouring rule each ---------------------------------------------------------------

class ArmsBeforeMoves(FullDriver):
    """(a) A batch arms its records before its moves."""
    def _after_batch(self, ops, cands, flagged, st):
        for h in flagged:
            self._arm(h, st)
        self._batch_ops(ops, cands, st)


class MergeKeepsStored(FullDriver):
    """(b) A same-version merge with an auto entry keeps the stored due time instead of the minimum."""
    def _kept(self, fn, h, *a):
        before = self.entries.get(int(h)) if h != NONE else None
        out = fn(h, *a)
        after = self.entries.get(int(h)) if h != NONE else None
        if before is not None and after is not None and before[0] == after[0]:
            self.entries[int(h)] = before
        return out

    def _arm(self, h, st):
        return self._kept(super()._arm, h, st)

    def _auto_arm(self, h, src, transient, st):
        return self._kept(super()._auto_arm, h, src, transient, st)


class MoveLeavesCodes(FullDriver):
    """(c) A move does not copy the three delay codes to the detached handle."""
    def _move(self, s, d, st):
        tabs = (self.delay, self.adelay, self.tdelay)
        saved = [t.pop(int(s), None) for t in tabs]
        super()._move(s, d, st)
        for t, v in zip(tabs, saved):
            if v is not None:
                t[int(s)] = v


class FireNeedsDelayStarted(FullDriver):
    """(d) The fire rule demands InvalidationDelayStarted of auto entries too."""
    def _fires(self, st, h, v, auto):
        return super()._fires(st, h, v, 0)


class ReleaseLeavesEntry(FullDriver):
    """(e) fgi_release leaves the handle's timer entry."""
    def _drop_entry(self, h):
        return False


class ArmsAtOwnHandle(FullDriver):
    """(f) A SET_OUTPUT item is auto-armed at its own handle, not where its node lives when the batch ends."""
    def _resolve(self, cand, h):
        return h


class SubsStayWithSlot(FullDriver):
    """(g) Subscriptions stay with the slot on displacement."""
    def _move_subs(self, s, d):
        pass


class DeliveredStays(FullDriver):
    """(h) A delivered subscription stays in the table."""
    def _take(self, h):
        return list(self.subs.get(h, []))


MUTANTS = [ArmsBeforeMoves, MergeKeepsStored, MoveLeavesCodes, FireNeedsDelayStarted, ReleaseLeavesEntry,
           ArmsAtOwnHandle, SubsStayWithSlot, DeliveredStays]


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: m.__name__)
def test_a_neighbouring_rule_ends_elsewhere(mutant):
    told = [seed for seed in SEEDS if W.full_walk(mutant, seed)[0].fingerprint() != _walked(seed)[0].fingerprint()]
    assert told, f"no seed tells the model from: {mutant.__doc__}"
