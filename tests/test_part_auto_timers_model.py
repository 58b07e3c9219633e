"""The auto-invalidation timers per rank of a partition (fgi.h, C-ABI 0.14) as a model: test_part_timers_model.py's
handle map and collective tick with test_auto_timers_model.py's rules, and the scenarios
test_gpu_part_auto_timers.py drives the engine through. This file runs the model alone (no GPU) and checks that no
scenario is vacuous.

`PartAutoDriver` is `PartDriver` and `AutoDriver` at once. What it adds of its own:
  * tick: the partition's tick (fired slots are the wave's roots, fired detached handles are reported and not
    applied to the oracle) with the 0.13 fire rule (Consistent and (DelayStarted or auto)); fired_auto counts the
    auto entries fired on slots and on detached handles alike.
  * batch: the partition's own rule, step by step. A SET_OUTPUT step auto-arms behind its own cascade on the states
    that step left, at the item's own slot; a BEGIN_COMPUTE step applies its moves (kind included, then the delay
    arm with the min merge) when it runs; the delay arm rule runs once at the end over everything the batch's
    cascades flagged, on the states the batch left. So a node that a later step invalidates keeps a stale entry
    (dropped when it comes due), where the single device's batch of 0.13 reads end-of-batch states and stores none.
Every scenario's graph is padded with empty slots (`pad_arrays`) so that n is not a multiple of P, the last rank
is short and no rank is empty. Expected values never come from the engine; the one thing the model takes from it
is which detached handle a displaced node was given."""
import functools

import numpy as np

import fgo as O
from harness import COMPUTING, CONSISTENT, F_DS, F_HD, F_IOSO, INVALIDATED
from test_gpu_flagged import expected_flagged
import test_auto_timers_model as A
from test_auto_timers_model import AUTO, _entry, slot_arrays
import test_part_timers_model as PM
import test_timers_model as M
from test_timers_model import NEVER, NONE, _u32

RANKS = (2, 3)


class PartAutoDriver(PM.PartDriver, A.AutoDriver):
    def __init__(self, arrays, n_det, P, default_delay=0, now=0, engine=None, fgi=None, default_auto=0, default_transient=0):
        super().__init__(arrays, n_det, P, default_delay=default_delay, now=now, engine=engine, fgi=fgi)
        self.def_auto, self.def_trans = default_auto, default_transient
        self.seen.update(det_fired_auto=0, batch_stale=0, batch_moved_auto=0, batch_overwrites=0)

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
            auto = self.kind[h] & AUTO
            live = st[0][h] != 0 and (st[1][h] & 3) == CONSISTENT and int(st[0][h]) == v
            if live and (auto or (st[1][h] & F_DS)):
                (roots if h < self.n else detached).append(h)
                self.ca["fired_auto"] += int(auto != 0)
                self.seen["fired_without_ds"] += int(not (st[1][h] & F_DS))
                self.seen["det_fired_auto"] += int(auto != 0 and h >= self.n)
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

    def batch(self, steps):
        """fgi_part_run_batch: the module docstring's rule."""
        got = outs = None
        if self.g:
            got, outs = self.g.run_batch(steps)
        flagged, want, armed = [], [], []
        for k, sp in enumerate(steps):
            before = self.states()
            step_inv = []
            if sp[0] == "invalidate":
                self._oracle_wave(sp[1], sp[2] if len(sp) > 2 else None)
            elif sp[0] == "begin_compute":
                handles = outs[k] if outs is not None else None
                moves, step_inv = self._oracle_begin(sp[1], sp[2], sp[3] if len(sp) > 3 else None, handles)
                st = self.states()
                for s, d in moves:
                    e = self.entries.get(s)
                    self.seen["batch_moved_auto"] += int(e is not None and e[0] == int(st[0][d]) and (self.kind[s] & AUTO) != 0)
                    self._move(s, d, st)
            elif sp[0] == "add_used":
                for d, u in zip(_u32(sp[1]), _u32(sp[2])):
                    self.o.add_used(self._node(d), self._node(u))
                continue
            elif sp[0] == "set_output":
                hs = _u32(sp[1])
                tr = np.zeros(len(hs), np.uint8) if len(sp) < 3 or sp[2] is None else np.asarray(sp[2], np.uint8)
                codes = self._codes(hs, before, set())
                if outs is not None:
                    assert list(outs[k]) == [int(c != 0) for c in codes], f"step {k}: out differs (it stays 0 / 1)"
                for h in hs:
                    self.o.set_output(self._node(h))
                st = self.states()
                if self.auto:
                    over = self.seen["overwrites"]
                    for h, c, t in zip(hs, codes, tr):
                        if c == 1:
                            self._auto_arm(h, h, t, st)
                            armed.append((int(h), int(st[0][h])))
                    self.seen["batch_overwrites"] += self.seen["overwrites"] - over
            after = self.states()
            flagged += list(expected_flagged(before, after)[0])
            want.append(np.sort(np.append(self._invalidated(before, after), step_inv).astype(np.uint32)))
        st = self.states()
        for h, v in armed:   # armed by a step, and the batch went on to invalidate or replace the node under the entry
            e = self.entries.get(h)
            if e is not None and e[0] == v and (int(st[0][h]) != v or (st[1][h] & 3) != CONSISTENT):
                self.seen["batch_stale"] += 1
        for h in flagged:
            self._arm(h, st)
        want = np.concatenate(want).astype(np.uint32) if want else np.zeros(0, np.uint32)
        if self.g:
            assert len(got) == len(want) and np.array_equal(np.sort(got), np.sort(want)), f"the batch's ids: {len(got)} vs {len(want)}"
        self.check()
        return want


def padded_n(n, P):
    """The smallest n' >= n that is no multiple of P and leaves no rank of P empty."""
    while n % P == 0 or n < 2 * P + 1:
        n += 1
    return n


def pad_arrays(arrays, P):
    versions, flags, src, dst, tags = arrays
    n = padded_n(len(versions), P)
    if n == len(versions):
        return arrays
    v, f = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    v[:len(versions)], f[:len(flags)] = versions, flags
    return v, f, src, dst, tags


def _alone(P):
    return lambda arrays, n_det, **kw: PartAutoDriver(pad_arrays(arrays, P), n_det, P, **kw)


# ---- the partition's own scenarios: make(arrays, n_det, **kw) -> PartAutoDriver ----------------------------------

def scn_part_displacement(make):
    """X1 (slot 1) and X2 (slot 7, another rank), delayed with delay 4, and Z (slot 2, no delay), all with auto
    entries due 20, displaced at now 3. The X entries move to their owners' detached handles, kind kept, and the
    delay arm behind the move brings them to 7. tick(7) fires both THERE: reported, not cascaded, the node words
    unchanged, fired_auto counted. Z's stale entry leaves at its due time."""
    drv = make(slot_arrays(8), 2)
    drv.open()
    drv.auto_open()
    drv.set_auto_delay([1, 2, 7], [20, 20, 20], [6, 6, 6])
    drv.set_delay([1, 7], [4, 4])
    drv.begin_compute([1, 2, 7], [51, 52, 57], [1, 0, 1])
    drv.set_output([1, 2, 7])
    assert all(_entry(drv, h) == (50 + h, 20, AUTO) for h in (1, 2, 7))
    drv.set_now(3)
    moved = drv.begin_compute([1, 2, 7], [61, 62, 67])
    assert len(moved) == 2 and drv.owner(moved[0]) == drv.owner(1) != drv.owner(7) == drv.owner(moved[1])
    d1, d7 = moved
    assert _entry(drv, d1) == (51, 7, AUTO) and _entry(drv, d7) == (57, 7, AUTO)
    assert drv.c["moved"] == 2 and drv.ca["merged"] == 2 and set(drv.entries) == {d1, d7, 2}
    assert drv.adelay[d7] == 20 and drv.tdelay[d7] == 6    # the codes went with the node
    before = drv.states()
    ids, fired = drv.tick(7)
    assert len(ids) == 0 and fired == 2 and sorted(sum(drv.ticks[-1][1], [])) == [d1, d7] and drv.ticks[-1][0] == [0] * drv.P
    assert drv.ca["fired_auto"] == 2 and drv.c["runs"] == 0
    after = drv.states()
    assert np.array_equal(before[1], after[1]) and (after[1][d1] & 3) == CONSISTENT   # the host ends such a node itself
    drv.release([d1, d7])
    dropped = drv.c["dropped"]
    assert drv.tick(20)[1] == 0 and drv.c["dropped"] == dropped + 1 and not drv.entries
    return drv


def scn_part_batch(make):
    """Three batches under the partition's step-by-step rule.
    (1) step 0 sets slots 1 (delayed) and 2, step 1 computes both again: both are armed at their slots behind step
        0; slot 1's entry moves with its node (kind kept, the delay arm merges 31 against 10), slot 2's node dies
        and its entry stays behind, stale.
    (2) step 0 sets slot 3, step 1 invalidates it: the entry armed behind step 0 stays, stale.
    (3) set 4 and 5 (5 transient), compute both again, set both again: slot 4's second arm overwrites the stale
        entry of its first node, slot 5's first node lives on under a detached handle with the transient entry."""
    drv = make(slot_arrays(8), 4, default_transient=2)
    drv.open()
    drv.auto_open()
    drv.set_auto_delay([1, 2, 3, 4, 5], [9, 9, 9, 9, 9])
    drv.set_delay([1, 5], [30, 30])
    drv.begin_compute([1, 2, 3, 4, 5], [71, 72, 73, 74, 75], [1, 0, 0, 0, 1])
    drv.set_now(1)
    drv.batch([("set_output", [1, 2]), ("begin_compute", [1, 2], [81, 82])])
    d1 = max(drv.entries)
    assert d1 >= drv.n and _entry(drv, d1) == (71, 10, AUTO) and _entry(drv, 2) == (72, 10, AUTO) and len(drv.entries) == 2
    assert drv.ca == dict(armed_auto=2, merged=1, fired_auto=0) and drv.c["moved"] == 1
    assert drv.seen["batch_moved_auto"] == 1 and drv.seen["batch_stale"] == 1
    drv.batch([("set_output", [3]), ("invalidate", [3], [1])])
    assert _entry(drv, 3) == (73, 10, AUTO) and (drv.states()[1][3] & 3) == INVALIDATED and drv.seen["batch_stale"] == 2
    drv.set_now(2)
    drv.batch([("set_output", [4, 5], [0, 1]), ("begin_compute", [4, 5], [84, 85], [0, 1]), ("set_output", [4, 5])])
    d5 = max(drv.entries)
    assert d5 >= drv.n and d5 != d1
    assert {h: _entry(drv, h) for h in drv.entries if h not in (d1, 2, 3)} == {
        4: (84, 11, AUTO), 5: (85, 11, AUTO), d5: (75, 4, AUTO)}     # d5: transient (2), merged with its delay (32)
    assert drv.seen["batch_overwrites"] == 1 and drv.seen["batch_moved_auto"] == 2 and drv.c["dropped"] == 1
    dropped = drv.c["dropped"]
    assert drv.tick(4)[1] == 1                            # d5, on its detached handle
    ids, fired = drv.tick(10)                             # d1 fires; the entries of slots 2 and 3 are stale
    assert fired == 1 and len(ids) == 0 and drv.c["dropped"] == dropped + 2
    ids, fired = drv.tick(11)
    assert fired == 2 and list(ids) == [4, 5] and not drv.entries
    return drv


DIV_N, DIV_HUB = 200, 0


def divergence_order(n, P):
    """Every slot once, ordered so that consecutive items belong to different ranks: within any run of 64 items
    owned and unowned slots alternate for every rank."""
    block = -(-n // P)
    return np.array([r * block + i for i in range(block) for r in range(P) if r * block + i < n], np.uint32)


def scn_divergence(make, P):
    """200 slots (padded for P), one list for every rank in which the owners alternate item by item. By slot % 4: 0
    freshly begun; 1 freshly begun, then flagged InvalidateOnSetOutput by a cascade from the hub; 2 empty (unset; slot
    2 itself holds a node the hub's cascade invalidates);
    3 freshly begun and transient. Every eighth slot has no auto delay (never). set_output with the whole list,
    then start_auto with the whole list (merges on the stored entries, skips what is not Consistent)."""
    drv = make(slot_arrays(DIV_N, consistent=[DIV_HUB, 2], edges=[(DIV_HUB, 2)]), 0, default_auto=6, default_transient=2)
    n = drv.n
    order = divergence_order(n, P)
    assert len(order) == n and len(set(order.tolist())) == n
    drv.open()
    drv.auto_open()
    s = np.arange(1, DIV_N, dtype=np.uint32)
    begun = s[s % 4 != 2]
    ioso = s[s % 4 == 1]
    drv.set_auto_delay(s[s % 8 == 0], np.full(int((s % 8 == 0).sum()), NEVER, np.uint64))
    drv.begin_compute(begun, begun.astype(np.uint64) + np.uint64(500))
    drv.add_used(ioso, np.full(len(ioso), DIV_HUB, np.uint32))
    assert list(drv.invalidate([DIV_HUB])) == [DIV_HUB, 2]   # (slot 2: registered in bulk under the hub, so that codes exist)
    assert all((drv.states()[1][h] & F_IOSO) for h in ioso)
    drv.set_output(order, transient=(order % 4 == 3).astype(np.uint8))
    plain, trans = s[(s % 4 == 0) & (s % 8 != 0)], s[s % 4 == 3]
    assert set(drv.entries) == set(plain.tolist()) | set(trans.tolist())
    assert all(drv.entries[h][1] == 6 for h in plain) and all(drv.entries[h][1] == 2 for h in trans)
    drv.set_now(1)
    drv.start_auto(order, transient=(order % 5 == 0).astype(np.uint8))
    ids, fired = drv.tick(2)
    assert fired == len(trans)
    drv.tick(3)
    drv.tick(7)
    assert not drv.entries
    return drv


GRID_P = 2
GRID_N = 600_001            # block 300,001: rank 0 owns 300,001 slots, rank 1 the other 300,000
GRID_A = 300_001            # registered Consistent in bulk: rank 0's slots


@functools.lru_cache(maxsize=None)
def _grid_arrays():
    versions = np.zeros(GRID_N, np.uint64)
    versions[:GRID_A] = O.version_of(47, np.arange(GRID_A, dtype=np.uint64))
    flags = np.zeros(GRID_N, np.uint32)
    flags[:GRID_A] = CONSISTENT
    none = np.zeros(0, np.uint32)
    arrays = (versions, flags, none, none, np.zeros(0, np.uint64))
    for a in arrays:
        a.setflags(write=False)
    return arrays


def scn_part_past_one_grid(make):
    """Two ranks over 600,001 slots. start_auto over rank 0's 300,001 Consistent slots and set_output of rank 1's
    300,000 freshly begun ones, each list handed whole to both ranks: on the rank that owns it k_tm_arm_auto_part
    strides past its grid of at most 1,024 x 256 lanes (the last wavefront partial), on the other rank every item
    is skipped. Every fifth item transient (due 2, the others 6)."""
    drv = make(_grid_arrays(), 0, default_auto=6, default_transient=2)
    assert drv.n == GRID_N and drv.P == GRID_P and drv.block == GRID_A
    drv.open()
    drv.auto_open()
    a = np.arange(GRID_A, dtype=np.uint32)
    b = np.arange(GRID_A, GRID_N, dtype=np.uint32)
    drv.start_auto(a, (a % 5 == 0).astype(np.uint8))
    assert len(drv.entries) == GRID_A
    drv.begin_compute(b, b.astype(np.uint64) + np.uint64(7))
    drv.set_output(b, transient=(b % 5 == 0).astype(np.uint8))
    assert len(drv.entries) == GRID_N
    n_tr = int((a % 5 == 0).sum() + (b % 5 == 0).sum())
    ids, fired = drv.tick(2)
    assert fired == n_tr and drv.ticks[-1][0] == [int((a % 5 == 0).sum()), int((b % 5 == 0).sum())]
    ids, fired = drv.tick(6)
    assert fired == GRID_N - n_tr and not drv.entries
    return drv


def scn_parity(make):
    """Single calls only (no multi-step batch, no displacement), for the comparison with a single device: default
    and per-slot delays, transient flags, a delay entry merged into an auto one, a tick, start_auto."""
    n = 24
    drv = make(slot_arrays(n, consistent=[0]), 0, default_auto=7, default_transient=3, now=10)
    drv.open()
    drv.auto_open()
    hs = np.arange(1, n, dtype=np.uint32)
    drv.set_auto_delay([2, 5, 13, 20], [5, NEVER, 40, 5], [0, 0, 0, 1])
    drv.set_delay([12, 13, 14], [2, 2, 50])
    drv.begin_compute(hs, hs.astype(np.uint64) + np.uint64(300), (hs >= 12).astype(np.uint8))
    dep = np.arange(12, 18, dtype=np.uint32)
    drv.add_used(dep, np.zeros(len(dep), np.uint32))
    drv.set_output(hs, transient=(hs % 3 == 0).astype(np.uint8))
    drv.set_now(11)
    assert list(drv.invalidate([0])) == [0]               # flags 12..17: delay arms merge into the auto entries
    assert drv.ca["merged"] >= 3
    drv.tick(13)
    drv.start_auto(hs[::2], transient=(hs[::2] % 4 == 0).astype(np.uint8))
    drv.tick(15)
    drv.tick(17)
    return drv


class ProcPlan:
    """What the two-process test's ranks (tests/part_auto_timers_worker.py) and the model run on: 11 empty slots
    over two ranks (block 6), two detached handles each. Six slots are computed and set, two of them transient
    (due 2, the others 6); tick(2) fires one entry on each rank; at 3 slot 3's node (delayed, delay 2) is displaced:
    its auto entry moves and the delay arm brings it to 5; tick(5) fires it on its detached handle; tick(6) fires
    the rest."""
    N, N_DET = 11, 2
    DEFAULTS = dict(default_auto=6, default_transient=2)
    SLOTS = np.array([1, 2, 3, 7, 8, 9], np.uint32)
    VERSIONS = SLOTS.astype(np.uint64) + np.uint64(40)
    HAS_DELAY = np.array([0, 0, 1, 0, 0, 0], np.uint8)
    TRANSIENT = np.array([1, 0, 0, 1, 0, 0], np.uint8)
    AUTO_DELAYS = np.array([0, 0, 0, 0, 0, 6], np.uint64)
    TRANS_DELAYS = np.array([2, 0, 0, 0, 0, 0], np.uint64)
    DELAYED, DELAY = np.array([3], np.uint32), 2
    MOVE_AT = 3
    MOVED = np.array([3], np.uint32)
    MOVED_VERSIONS = np.array([90], np.uint64)
    TICKS = (2, 5, 6)

    @staticmethod
    def arrays():
        return slot_arrays(ProcPlan.N)


INHERITED = ("scn_chain", "scn_selection", "scn_no_defaults", "scn_ioso_delay", "scn_merge", "scn_delay_then_auto",
             "scn_cascading", "scn_start_auto")


# ---- the model alone ------------------------------------------------------------------------------------------

def _identity(drv):
    c = drv.c
    assert c["armed"] == c["fired"] + c["dropped"] + len(drv.entries), c


@functools.lru_cache(maxsize=None)
def _run(name, P):
    return getattr(A, name)(_alone(P))


def test_padding():
    assert [padded_n(4, P) for P in RANKS] == [5, 7] and [padded_n(200, P) for P in RANKS] == [201, 200]
    assert padded_n(4096, 2) == 4097 and padded_n(4096, 3) == 4096 and padded_n(GRID_N, GRID_P) == GRID_N
    for n, P in ((5, 2), (7, 3), (201, 2), (200, 3), (4097, 2), (4096, 3)):
        block = -(-n // P)
        assert 0 < n - (P - 1) * block < block, "the last rank is short and not empty"


def test_inherited_scenarios_model():
    """0.13's scenarios that hand out no detached handle, over P ranks: the same counters as on one device."""
    for P in RANKS:
        assert _run("scn_chain", P).ca == dict(armed_auto=1, merged=0, fired_auto=1)
        assert _run("scn_chain", P).seen["fired_without_ds"] == 1
        sel = _run("scn_selection", P)
        assert sel.ca == dict(armed_auto=7, merged=0, fired_auto=6) and sel.seen["overwrites"] >= 1 and sel.seen["auto_none"] == 2
        assert _run("scn_no_defaults", P).seen["auto_none"] >= 3
        assert _run("scn_ioso_delay", P).seen["ioso"] == 1 and _run("scn_ioso_delay", P).ca["armed_auto"] == 0
        assert _run("scn_merge", P).ca == dict(armed_auto=2, merged=3, fired_auto=2)
        assert _run("scn_delay_then_auto", P).ca == dict(armed_auto=0, merged=1, fired_auto=1)
        assert _run("scn_cascading", P).ca == dict(armed_auto=1, merged=0, fired_auto=1) and _run("scn_cascading", P).c["runs"] == 2
        sa = _run("scn_start_auto", P)
        assert sa.ca["merged"] >= 3 and sa.ca["fired_auto"] >= 1000 and sa.seen["not_consistent"] >= 100 and sa.seen["stale"] >= 1
        both = sum(1 for roots, _ in sa.ticks if sum(1 for x in roots if x) >= 2)
        assert both >= 1, "no tick in which two ranks fire auto entries"
        for name in INHERITED:
            _identity(_run(name, P))
            assert _run(name, P).n % P != 0


def test_displacement_model():
    for P in RANKS:
        drv = scn_part_displacement(_alone(P))
        assert drv.seen["det_fired_auto"] == 2 and drv.seen["det_moved"] == 2 and drv.seen["stale"] == 1
        assert [len(d) for d in drv.ticks[0][1]].count(1) == 2, "two owners' detached handles fire"
        _identity(drv)


def test_batch_model():
    for P in RANKS:
        drv = scn_part_batch(_alone(P))
        assert drv.seen["batch_stale"] == 2 and drv.seen["batch_moved_auto"] == 2 and drv.seen["batch_overwrites"] == 1
        assert drv.seen["stale"] == 2 and drv.seen["det_fired_auto"] == 2
        assert drv.ca == dict(armed_auto=7, merged=2, fired_auto=4)
        _identity(drv)


def test_batch_rule_differs_from_the_single_device():
    """The same steps under 0.13's end-of-batch rule store no stale entry: the two models must not be confused."""
    part, one = scn_part_batch(_alone(2)), A.scn_batch(A._alone)
    assert part.ca["armed_auto"] == 7 and one.ca["armed_auto"] == 4
    assert part.c["dropped"] == 3 and one.c["dropped"] == 0


def test_divergence_model():
    for P in RANKS:
        drv = scn_divergence(_alone(P), P)
        order = divergence_order(drv.n, P)
        for r in range(P):                                 # in every full run of 64 items every rank owns some, not all
            mine = (order // drv.block) == r
            runs = [mine[i:i + 64] for i in range(0, len(order) - 63, 64)]
            assert len(runs) >= 3 and all(0 < int(x.sum()) < 64 for x in runs), (P, r)
        s = drv.seen
        assert s["ioso"] == 50 and s["unset"] >= 50 and s["auto_none"] >= 20 and s["not_consistent"] >= 100
        assert drv.ca["merged"] >= 50 and drv.ca["armed_auto"] >= 75 and drv.ca["fired_auto"] >= 75
        _identity(drv)


def test_parity_model():
    for P in RANKS:
        drv = scn_parity(_alone(P))
        assert drv.ca["merged"] >= 3 and drv.ca["fired_auto"] >= 10 and drv.seen["auto_none"] >= 1 and not drv.det
        assert drv.seen["fired_without_ds"] >= 1
        _identity(drv)


def test_proc_plan_model():
    """The two-process test's plan on the model alone: both ranks fire at the first tick, one auto entry moves and
    fires on its detached handle, the rest fire as roots."""
    W = ProcPlan
    drv = PartAutoDriver(W.arrays(), W.N_DET, 2, **W.DEFAULTS)
    assert padded_n(W.N, 2) == W.N and drv.block == 6
    drv.open()
    drv.auto_open()
    drv.set_auto_delay(W.SLOTS, W.AUTO_DELAYS, W.TRANS_DELAYS)
    drv.set_delay(W.DELAYED, [W.DELAY] * len(W.DELAYED))
    drv.begin_compute(W.SLOTS, W.VERSIONS, W.HAS_DELAY)
    drv.set_output(W.SLOTS, transient=W.TRANSIENT)
    assert len(drv.entries) == 6 and sorted(t for _, t in drv.entries.values()) == [2, 2, 6, 6, 6, 6]
    assert drv.tick(W.TICKS[0])[1] == 2 and drv.ticks[-1][0] == [1, 1]
    drv.set_now(W.MOVE_AT)
    (d,) = drv.begin_compute(W.MOVED, W.MOVED_VERSIONS)
    assert _entry(drv, d) == (43, 5, AUTO) and drv.c["moved"] == 1 and drv.ca["merged"] == 1
    ids, fired = drv.tick(W.TICKS[1])
    assert len(ids) == 0 and fired == 1 and drv.seen["det_fired_auto"] == 1
    ids, fired = drv.tick(W.TICKS[2])
    assert list(ids) == [2, 8, 9] and fired == 3 and not drv.entries
    assert drv.ca == dict(armed_auto=6, merged=1, fired_auto=6)
    _identity(drv)


def test_past_one_grid_model():
    drv = scn_part_past_one_grid(_alone(GRID_P))
    assert GRID_N % GRID_P != 0 and drv.block == 300_001 and GRID_N - drv.block == 300_000
    assert min(GRID_A, GRID_N - GRID_A) > M.GRID_LANES == 1024 * 256 and GRID_A % 64 != 0 and (GRID_N - GRID_A) % 64 != 0
    assert [t[1:] for t in drv.trace if t[0] == "start_auto"] == [(GRID_A,)]
    assert (GRID_N - GRID_A,) in [t[1:] for t in drv.trace if t[0] == "set_output"]
    assert drv.ca == dict(armed_auto=GRID_N, merged=0, fired_auto=GRID_N)
    _identity(drv)
