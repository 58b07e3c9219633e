"""The delay timers per rank of a partition (fgi.h, C-ABI 0.12) as the model of test_timers_model.py over P ranks,
and the scenario test_gpu_part_timers.py adds for the partition's own edges. This file runs the model alone (no
GPU) and checks that the scenarios are not vacuous.

`PartDriver` is `Driver` with another handle map and another tick:
  * Model handles [0, n) are the host's global slots; detached handle d of rank r (a local handle of that rank,
    d >= block) is model handle n + r * n_det + (d - block). Alone, the model gives a displaced node the lowest
    free detached handle of the slot's owner; with an engine it takes the handle the owner handed out.
  * tick: the due entries of detached handles that pass the fire test are removed and counted as fired, per
    owner, but are not applied to the oracle (no partitioned cascade reaches a detached node: the host ends such
    a node itself). The wave's roots are the fired slots only; without one no wave runs and `runs` stays.
`begin_compute`, `invalidate`, `set_output`, `release`, `_arm` and `_move` are inherited unchanged, and so is
`batch`'s rule (the steps one by one, then the moves in step order, then the arm rule once on the states the
batch left): a partition arms once per call, behind its last cascade and its moves. `batch` itself is wrapped in
one respect: an in-process batch returns its ids rank by rank with no step boundaries (every partition test
compares them as a multiset), so the model's batch runs on the detached handles the engine handed out and the ids
are compared sorted.

The engine is reached through a small adapter (`engine`: Graph-like calls over the group, written in
test_gpu_part_timers.py) whose handles are model handles."""
import numpy as np

from harness import COMPUTING, CONSISTENT, F_HD
from test_gpu_flagged import expected_flagged
import test_timers_model as M

NONE = M.NONE


class PartDriver(M.Driver):
    def __init__(self, arrays, n_det, P, default_delay=0, now=0, engine=None, fgi=None):
        super().__init__(arrays, P * n_det, default_delay=default_delay, now=now, engine=engine, fgi=fgi)
        self.P, self.rank_det = P, n_det
        self.block = -(-self.n // P)
        self.free = []                     # unused: the owner's range decides (_alone_handles)
        self._fed = None
        self.seen.update(det_fired=0, det_moved=0)
        # per tick: (roots per rank, fired detached handles per rank)
        self.ticks = []

    # ---- the handle map ----
    def owner(self, h):
        h = int(h)
        return h // self.block if h < self.n else (h - self.n) // self.rank_det

    def _alone_handles(self, slots):
        """The model alone: which of the call's slots displace a node that lives on (Computing, or Consistent with
        an InvalidationDelay), each given the lowest free detached handle of its owner."""
        v, f = self.states()
        taken, out = set(self.det), []
        for s in M._u32(slots):
            s = int(s)
            lives = v[s] != 0 and ((f[s] & 3) == COMPUTING or ((f[s] & 3) == CONSISTENT and (f[s] & F_HD) != 0))
            d = NONE
            if lives:
                lo = self.n + self.owner(s) * self.rank_det
                d = next(x for x in range(lo, lo + self.rank_det) if x not in taken)
                taken.add(d)
            out.append(d)
        return np.array(out, np.uint32)

    def _oracle_begin(self, slots, versions, has_delay, handles):
        if handles is None:
            handles = self._fed.pop(0) if self._fed else self._alone_handles(slots)
        moves, inv = super()._oracle_begin(slots, versions, has_delay, handles)
        for s, d in moves:
            assert self.owner(s) == self.owner(d), f"slot {s}'s node went to detached handle {d} of another rank"
        self.seen["det_moved"] += sum(1 for s, _ in moves if s in self.entries)
        return moves, inv

    def batch(self, steps):
        if not self.g:
            return super().batch(steps)
        eng = self.g
        got, outs = eng.run_batch(steps)
        self.g, self._fed = None, [outs[k] for k, sp in enumerate(steps) if sp[0] == "begin_compute"]
        try:
            want = super().batch(steps)
        finally:
            self.g, self._fed = eng, None
        assert len(got) == len(want) and np.array_equal(np.sort(got), np.sort(want)), f"the batch's ids: {len(got)} vs {len(want)}"
        self.check()
        return want

    # ---- the collective tick ----
    def tick(self, now):
        """fgi_part_timers_run_due(now) on every rank: (ids of the fired timers' wave, entries fired on all ranks)."""
        assert now >= self.now
        self.now = now
        st = self.states()
        due = sorted(h for h, (_, t) in self.entries.items() if t <= now)
        stored = len(self.entries)
        roots, detached = [], []
        for h in due:
            v, _ = self.entries.pop(h)
            if self._waiting(st, h) and int(st[0][h]) == v:
                (roots if h < self.n else detached).append(h)
            else:
                self.c["dropped"] += 1
                self.seen["stale"] += 1
        self.c["fired"] += len(roots) + len(detached)
        self.seen["det_fired"] += len(detached)
        self.trace.append(("tick", stored, len(roots) + len(detached)))
        self.ticks.append(([sum(1 for h in roots if self.owner(h) == r) for r in range(self.P)],
                           [[h for h in detached if self.owner(h) == r] for r in range(self.P)]))
        want = np.zeros(0, np.uint32)
        if roots:
            self.c["runs"] += 1
            self._oracle_wave(roots, np.ones(len(roots), np.uint8))
            after = self.states()
            for h in expected_flagged(st, after)[0]:
                self._arm(h, after)
            want = self._invalidated(st, after)
        if self.g:
            self.g.tick(now, want if roots else None, *self.ticks[-1])
        self.check()
        return want, len(roots) + len(detached)


def _alone(P):
    return lambda arrays, n_det, **kw: PartDriver(arrays, n_det, P, **kw)


# ---- the partition's own edges --------------------------------------------------------------------------------
EDGE_N, EDGE_P, EDGE_DET, EDGE_HUB = 200, 3, 8, 100
EDGE_TICK1 = list(range(140, 150))                     # rank 2 only
EDGE_MOVED = [5, 150]                                  # displaced with stored entries: rank 0, rank 2
EDGE_TICK3 = [67, 134, 199]                            # the first slots of ranks 1 and 2, and the last slot


def edge_plan(n=EDGE_N, P=EDGE_P):
    """Slot 100 -> every other slot, every one of them delayed. Delays: 1 for ten slots of the last rank, 2 for
    rank 0's slots but one, 3 for that one, one slot of the last rank, the first slots of ranks 1 and 2 and the
    last slot, 50 for the rest. (At P = 2 the same lists fall on two ranks.)"""
    block = -(-n // P)
    others = np.array([h for h in range(n) if h != EDGE_HUB], np.uint32)
    arrays = M.chain_arrays(n, [(EDGE_HUB, int(h)) for h in others], delayed=others.tolist(), seed=17)
    delays = np.full(n, 50, np.uint64)
    delays[:min(block, 67)] = 2
    delays[EDGE_TICK1] = 1
    delays[EDGE_MOVED + EDGE_TICK3] = 3
    return arrays, others, delays


def scn_part_edges(make, n=EDGE_N, P=EDGE_P):
    arrays, others, delays = edge_plan(n, P)
    drv = make(arrays, EDGE_DET)
    drv.open()
    drv.set_delay(others, delays[others])
    assert list(drv.invalidate([EDGE_HUB])) == [EDGE_HUB] and len(drv.entries) == n - 1
    ids, fired = drv.tick(1)                               # (a) the last rank's entries only
    assert list(ids) == EDGE_TICK1 and fired == len(EDGE_TICK1)
    v = drv.states()[0]
    moved = drv.begin_compute(EDGE_MOVED, v[EDGE_MOVED] + np.uint64(10))
    assert len(moved) == 2 and drv.c["moved"] == 2 and [drv.owner(d) for d in moved] == [drv.owner(s) for s in EDGE_MOVED]
    ids, fired = drv.tick(2)                               # (b) 66 entries of rank 0, none elsewhere
    assert fired == 66 and {0, 63, 64, 66} <= set(ids.tolist()) and ids.max() <= 66
    ids, fired = drv.tick(3)                               # (c) three slots and the two displaced nodes
    assert list(ids) == EDGE_TICK3 and fired == 5 and sorted(sum(drv.ticks[-1][1], [])) == sorted(moved)
    runs = drv.c["runs"]
    ids, fired = drv.tick(4)                               # nothing due: no wave
    assert len(ids) == 0 and fired == 0 and drv.c["runs"] == runs
    ids, fired = drv.tick(50)
    assert fired == n - 1 - len(EDGE_TICK1) - 66 - 5 and not drv.entries
    return drv


# ---- the model alone ------------------------------------------------------------------------------------------

def test_edges_model():
    drv = scn_part_edges(_alone(EDGE_P))
    assert drv.block == 67 and drv.n - 2 * drv.block == 66
    t1, t2, t3 = drv.ticks[0], drv.ticks[1], drv.ticks[2]
    assert t1[0] == [0, 0, 10], "tick 1: ranks 0 and 1 join with zero roots"
    assert t2[0] == [66, 0, 0] and 66 > 64 and 66 % 64 != 0, "tick 2: more than one wavefront, the last one partial"
    assert t3[0] == [0, 1, 2] and [len(d) for d in t3[1]] == [1, 0, 1], "tick 3: two ranks' roots, two owners' detached"
    assert drv.seen["det_fired"] == 2 and drv.seen["det_moved"] == 2
    assert drv.c == dict(armed=199, fired=199, dropped=0, moved=2, runs=4)


def test_edges_model_two_ranks():
    """The same lists over two ranks (the two-process test's shape): block 100, the displaced slots on both."""
    drv = scn_part_edges(_alone(2), P=2)
    assert drv.ticks[0][0] == [0, 10] and drv.ticks[1][0] == [66, 0] and drv.ticks[2][0] == [1, 2]
    assert [len(d) for d in drv.ticks[2][1]] == [1, 1]


def test_inherited_scenarios_model():
    """The single-device scenarios apply unchanged where no detached handle fires."""
    for P in (1, 2):
        assert M.scn_chain(_alone(P)).c == dict(armed=1, fired=1, dropped=0, moved=0, runs=1)
        assert M.scn_cascading(_alone(P)).c == dict(armed=2, fired=2, dropped=0, moved=0, runs=2)
        assert M.scn_slot_reuse(_alone(P)).seen["stale"] == 1
        assert M.scn_saturation(_alone(P)).c == dict(armed=2, fired=2, dropped=0, moved=0, runs=1)
        M.scn_open_populated(_alone(P))


def _tick_kinds(drv):
    both = sum(1 for roots, _ in drv.ticks if sum(1 for x in roots if x) >= 2)
    lone = sum(1 for roots, _ in drv.ticks if any(roots) and not all(roots))
    return both, lone


def test_mixed_model_is_not_vacuous():
    for P in (2, 3, 8):
        drv = M.scn_mixed(_alone(P))
        c, s = drv.c, drv.seen
        both, _ = _tick_kinds(drv)
        assert both >= 1, "no tick in which two ranks contribute roots"
        assert c["fired"] >= 50 and s["stale"] >= 1 and s["overwrites"] >= 1 and c["moved"] >= 1 and s["never"] >= 1, (P, c, s)
        assert s["displaced_armed"] >= 1
        assert c["armed"] == c["fired"] + c["dropped"] + len(drv.entries)


def test_batch_model():
    for P in (2, 3):
        drv = M.scn_batch(_alone(P))
        assert drv.c["moved"] >= 8 and drv.seen["det_moved"] >= 8 and drv.c["fired"] >= 20
        assert drv.seen["det_fired"] >= 1, "no timer of a displaced leaf ran out under its detached handle"
        assert drv.c["armed"] == drv.c["fired"] + drv.c["dropped"] and not drv.entries


def test_scenarios_cover_the_tick_shapes():
    """What the issue asks the scenarios to hold, on the model alone: a tick with roots from two ranks, a tick in
    which one rank has none while another has some, a detached entry fired and one moved, a stale drop, an
    overwrite by another version, and the counter identity at the end."""
    edges = scn_part_edges(_alone(EDGE_P))
    mixed = M.scn_mixed(_alone(3))
    both = _tick_kinds(edges)[0] + _tick_kinds(mixed)[0]
    lone = _tick_kinds(edges)[1] + _tick_kinds(mixed)[1]
    assert both >= 1 and lone >= 1
    assert edges.seen["det_fired"] >= 1 and edges.seen["det_moved"] >= 1
    assert mixed.seen["stale"] >= 1 and mixed.seen["overwrites"] >= 1
    for drv in (edges, mixed):
        assert drv.c["armed"] == drv.c["fired"] + drv.c["dropped"] + len(drv.entries)
