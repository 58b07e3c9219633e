"""The auto-invalidation timers' semantics (fgi.h, C-ABI 0.13) as a model over test_timers_model.py's Driver and the
CPU oracle, and the scenarios test_gpu_auto_timers.py drives the engine through. This file runs the model alone
(no GPU) and checks that the scenarios are not vacuous.

`AutoDriver` adds to the delay timers' model: two more delays per handle (auto, transient error) and their
graph defaults, a kind per entry (bit 0: auto), the auto arm rule behind set_output (an item that went Computing ->
Consistent without InvalidateOnSetOutput) and behind start_auto, the min merge where an auto entry and a delay
arm of one version meet (AddOrUpdateToEarlier), the fire rule "Consistent and (DelayStarted or auto)", the delay
arm behind a moved auto entry, and a batch's walk over its steps with each SET_OUTPUT item resolved to the handle
where its node lives when the batch ends. Expected values never come from the engine."""
import functools

import numpy as np

import fgo as O
from harness import COMPUTING, CONSISTENT, F_DS, F_HD, F_IOSO, INVALIDATED
from test_gpu_flagged import N_DET as MIXED_DET, _mixed, expected_flagged
import test_timers_model as M
from test_timers_model import NEVER, NONE, _u32

AUTO = 1


class AutoDriver(M.Driver):
    def __init__(self, arrays, n_det, default_delay=0, now=0, engine=None, fgi=None, default_auto=0, default_transient=0):
        super().__init__(arrays, n_det, default_delay=default_delay, now=now, engine=engine, fgi=fgi)
        self.def_auto, self.def_trans = default_auto, default_transient
        self.adelay, self.tdelay = {}, {}
        self.kind = {}                     # handle -> kind of its entry (meaningful while the handle has one)
        self.auto = False
        self.ca = dict(armed_auto=0, merged=0, fired_auto=0)
        self.seen.update(ioso=0, unset=0, not_consistent=0, auto_none=0, fired_without_ds=0)

    # ---- the rules of fgi.h, 0.13 ----
    def _arm(self, h, st):
        """The delay arm rule over flagged records: as 0.11's, with the min merge into an auto entry."""
        h = int(h)
        if not self._waiting(st, h):
            return False
        d = self.delay.get(h, 0) or self.default
        if d == NEVER:
            self.seen["never"] += 1
            return False
        if d == 0:
            return False
        v = int(st[0][h])
        due = min(self.now + d, NEVER - 1)
        e = self.entries.get(h)
        if e is not None and e[0] == v:
            if self.kind[h] & AUTO:
                self.entries[h] = (v, min(e[1], due))
                self.ca["merged"] += 1
            return False                   # two delay arms of one version: the stored due time stays
        if e is not None:
            self.c["dropped"] += 1
            self.seen["overwrites"] += 1
        self.entries[h] = (v, due)
        self.kind[h] = 0
        self.c["armed"] += 1
        return True

    def _auto_arm(self, h, src, transient, st):
        """The auto arm rule for candidate h with the delays of handle src."""
        if h == NONE:
            return
        h, src = int(h), int(src)
        if st[0][h] == 0 or (st[1][h] & 3) != CONSISTENT:
            self.seen["not_consistent"] += 1
            return
        d = (self.tdelay.get(src, 0) or self.def_trans) if transient else (self.adelay.get(src, 0) or self.def_auto)
        if d == 0 or d == NEVER:
            self.seen["auto_none"] += 1
            return
        v = int(st[0][h])
        due = min(self.now + d, NEVER - 1)
        e = self.entries.get(h)
        if e is not None and e[0] == v:
            self.entries[h] = (v, min(e[1], due))
            self.kind[h] |= AUTO
            self.ca["merged"] += 1
            return
        if e is not None:
            self.c["dropped"] += 1
            self.seen["overwrites"] += 1
        self.entries[h] = (v, due)
        self.kind[h] = AUTO
        self.c["armed"] += 1
        self.ca["armed_auto"] += 1

    def _move(self, s, d, st):
        s, d = int(s), int(d)
        for tab in (self.delay, self.adelay, self.tdelay):
            if s in tab:
                tab[d] = tab[s]
            else:
                tab.pop(d, None)
        e = self.entries.get(s)
        if e is not None and st[0][d] != 0 and e[0] == int(st[0][d]):
            self.entries[d] = self.entries.pop(s)
            self.kind[d] = self.kind[s]
            self.c["moved"] += 1
            if self.kind[d] & AUTO:        # the displacement started the node's delay: the earlier due time stays
                self._arm(d, st)
        elif self._arm(d, st):
            self.seen["displaced_armed"] += 1

    def _codes(self, hs, st, done):
        """k_set_output's per-item code on states st: 0 not set, 1 set, 2 set on a node with InvalidateOnSetOutput
        (done: the handles an earlier item of the same call set already)."""
        codes = []
        for h in hs:
            h = int(h)
            is_set = h not in done and st[0][h] != 0 and (st[1][h] & 3) == COMPUTING
            if is_set:
                done.add(h)
            ioso = is_set and (st[1][h] & F_IOSO) != 0
            self.seen["ioso"] += int(ioso)
            self.seen["unset"] += int(not is_set)
            codes.append(2 if ioso else 1 if is_set else 0)
        return codes

    # ---- steps ----
    def auto_open(self):
        if self.g:
            self.g.timers_auto_open(self.def_auto, self.def_trans)
        self.auto = True
        self.check()

    def set_auto_delay(self, handles, auto=None, transient=None):
        for tab, ds in ((self.adelay, auto), (self.tdelay, transient)):
            if ds is None:
                continue
            for h, d in zip(_u32(handles), np.asarray(ds, np.uint64)):
                if int(d):
                    tab[int(h)] = int(d)
                else:
                    tab.pop(int(h), None)
        if self.g:
            self.g.timers_set_auto_delay(handles, auto, transient)
        self.check()

    def start_auto(self, handles, transient=None):
        hs = _u32(handles)
        tr = np.zeros(len(hs), np.uint8) if transient is None else np.asarray(transient, np.uint8)
        st = self.states()
        for h, t in zip(hs, tr):
            self._auto_arm(h, h, t, st)
        self.trace.append(("start_auto", len(hs)))
        if self.g:
            self.g.timers_start_auto(hs, transient)
        self.check()

    def set_output(self, handles, transient=None):
        hs = _u32(handles)
        tr = np.zeros(len(hs), np.uint8) if transient is None else np.asarray(transient, np.uint8)
        before = self.states()
        codes = self._codes(hs, before, set())
        for h in hs:
            self.o.set_output(self._node(h))
        after = self.states()
        for h in expected_flagged(before, after)[0]:
            self._arm(h, after)
        if self.auto:
            for h, c, t in zip(hs, codes, tr):
                if c == 1:
                    self._auto_arm(h, h, t, after)
        self.trace.append(("set_output", len(hs)))
        if self.g:
            got, _ = self.g.set_output(hs, transient=transient)
            assert list(got) == [int(c != 0) for c in codes], "out_set differs (it stays 0 / 1)"
        self.check()

    def tick(self, now):
        """fgi_timers_run_due(now) with the 0.13 fire rule: (ids of the fired timers' wave, entries fired)."""
        assert now >= self.now
        self.now = now
        st = self.states()
        due = sorted(h for h, (_, t) in self.entries.items() if t <= now)
        stored = len(self.entries)
        fire = []
        for h in due:
            v, _ = self.entries.pop(h)
            auto = self.kind[h] & AUTO
            live = st[0][h] != 0 and (st[1][h] & 3) == CONSISTENT and int(st[0][h]) == v
            if live and (auto or (st[1][h] & F_DS)):
                fire.append(h)
                self.ca["fired_auto"] += int(auto != 0)
                self.seen["fired_without_ds"] += int(not (st[1][h] & F_DS))
            else:
                self.c["dropped"] += 1
                self.seen["stale"] += 1
        self.c["fired"] += len(fire)
        self.trace.append(("tick", stored, len(fire)))
        want = np.zeros(0, np.uint32)
        if fire:
            self.c["runs"] += 1
            self._oracle_wave(fire, np.ones(len(fire), np.uint8))
            after = self.states()
            for h in expected_flagged(st, after)[0]:
                self._arm(h, after)
            want = self._invalidated(st, after)
        if self.g:
            got, fired = self.g.timers_run_due(now)
            assert fired == len(fire), f"fired {fired}, the model {len(fire)}"
            assert np.array_equal(got, want), f"the fired timers' wave: {len(got)} ids vs {len(want)}"
        self.check()
        return want, len(fire)

    def batch(self, steps):
        """fgi_run_batch: the steps on the oracle one by one. Behind them the steps are walked in order: a
        set_output step auto-arms (each item where its node lives when the batch ends, with its own handle's
        delays), a begin_compute step applies its moves; then the arm rule once over everything the cascades
        flagged. All on the states the batch left."""
        outs = None
        if self.g:
            got, outs = self.g.run_batch(steps)
        flagged, ops, want = [], [], []
        done = {}
        for k, sp in enumerate(steps):
            before = self.states()
            step_inv = []
            if sp[0] == "invalidate":
                self._oracle_wave(sp[1], sp[2] if len(sp) > 2 else None)
            elif sp[0] == "begin_compute":
                m, step_inv = self._oracle_begin(sp[1], sp[2], sp[3] if len(sp) > 3 else None,
                                                 outs[k] if outs is not None else None)
                ops.append(("begin", _u32(sp[1]), dict(m)))
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
                ops.append(("set", hs, codes, tr))
            after = self.states()
            flagged += list(expected_flagged(before, after)[0])
            want.append(np.sort(np.append(self._invalidated(before, after), step_inv).astype(np.uint32)))
        st = self.states()
        later, cands = {}, {}
        for i in range(len(ops) - 1, -1, -1):          # where each set_output item's node lives now
            if ops[i][0] == "begin":
                for s in ops[i][1]:
                    later[int(s)] = ops[i][2].get(int(s), NONE)
            else:
                cands[i] = [later.get(int(h), int(h)) for h in ops[i][1]]
        for i, op in enumerate(ops):
            if op[0] == "begin":
                for s, d in op[2].items():
                    self._move(s, d, st)
            elif self.auto:
                for h, c, t, cand in zip(op[1], op[2], op[3], cands[i]):
                    if c == 1:
                        self.seen["resolved_detached"] = self.seen.get("resolved_detached", 0) + int(cand not in (NONE, int(h)))
                        self.seen["resolved_none"] = self.seen.get("resolved_none", 0) + int(cand == NONE)
                        self._auto_arm(cand, h, t, st)
        for h in flagged:
            self._arm(h, st)
        want = np.concatenate(want).astype(np.uint32) if want else np.zeros(0, np.uint32)
        if self.g:
            assert np.array_equal(got, want), f"the batch's ids: {len(got)} vs {len(want)}"
        self.check()
        return want

    # ---- the engine against the model ----
    def kinds(self):
        return np.array([self.kind[h] for h in sorted(self.entries)], np.uint8)

    def check(self):
        super().check()
        if not self.g:
            return
        h, v, d, k = self.g.timers_list_ex()
        mh, mv, md = self.listed()
        assert np.array_equal(h, mh) and np.array_equal(v, mv) and np.array_equal(d, md), "fgi_timers_list_ex differs"
        bad = np.nonzero(k != self.kinds())[0]
        assert len(bad) == 0, f"kinds differ at handles {h[bad[:8]]}: engine {k[bad[:8]]}"
        want = self.ca if self.auto else dict(armed_auto=0, merged=0, fired_auto=0)
        assert self.g.timers_auto_stats() == want, (self.g.timers_auto_stats(), want)


def slot_arrays(n, consistent=(), delayed=(), computing=(), computing_delayed=(), edges=(), seed=41):
    """n slots, empty but for the listed ones; edges (used, dependant)."""
    versions = np.zeros(n, np.uint64)
    flags = np.zeros(n, np.uint32)
    for hs, f in ((consistent, CONSISTENT), (delayed, CONSISTENT | F_HD), (computing, COMPUTING),
                  (computing_delayed, COMPUTING | F_HD)):
        for h in hs:
            versions[h] = O.version_of(seed, np.array([h], np.uint64))[0]
            flags[h] = f
    src = np.array([e[0] for e in edges], np.uint32)
    dst = np.array([e[1] for e in edges], np.uint32)
    return versions, flags, src, dst, versions[dst] if len(dst) else np.zeros(0, np.uint64)


def _entry(drv, h):
    return drv.entries[h] + (drv.kind[h],)


# ---- scenarios: make(arrays, n_det, **kw) -> AutoDriver (with or without an engine) ------------------------------

def scn_chain(make):
    """begin / set_output A (auto 5); B begins, uses A and completes; tick(4) fires nothing, tick(5) fires A (which
    never had DelayStarted) and the wave invalidates B."""
    drv = make(slot_arrays(4), 0)
    drv.open()
    drv.auto_open()
    drv.set_auto_delay([0], [5])
    drv.begin_compute([0], [11])
    assert not drv.entries
    drv.set_output([0])
    assert _entry(drv, 0) == (11, 5, AUTO) and len(drv.entries) == 1
    drv.begin_compute([1], [12])
    drv.add_used([1], [0])
    drv.set_output([1])
    assert list(drv.entries) == [0]
    ids, fired = drv.tick(4)
    assert len(ids) == 0 and fired == 0
    ids, fired = drv.tick(5)
    assert list(ids) == [0, 1] and fired == 1 and not drv.entries
    return drv


def scn_selection(make):
    """Per-handle against default delays, the transient flag picks the other delay, NEVER stores nothing; then a
    slot computed again under its stale auto entry (an overwrite by another version)."""
    drv = make(slot_arrays(8), 0, default_auto=7, default_transient=3, now=100)
    drv.open()
    drv.auto_open()
    hs = np.arange(8, dtype=np.uint32)
    drv.set_auto_delay([0, 2, 6], [5, NEVER, 5])
    drv.set_auto_delay([4, 5], None, [2, NEVER])
    drv.begin_compute(hs, 20 + hs.astype(np.uint64))
    drv.set_output(hs, transient=[0, 0, 0, 1, 1, 1, 1, 0])
    due = {h: t for h, (_, t) in drv.entries.items()}
    # 0: its own auto delay; 1, 7: the default; 2: never; 3, 6: the transient default; 4: its own; 5: never
    assert due == {0: 105, 1: 107, 3: 103, 4: 102, 6: 103, 7: 107}
    assert all(drv.kind[h] == AUTO for h in drv.entries) and drv.seen["auto_none"] == 2
    drv.set_output(hs)                                   # already Consistent: not set, no candidates
    assert drv.ca == dict(armed_auto=6, merged=0, fired_auto=0)
    assert list(drv.invalidate([0], [1])) == [0]        # the entry stays (lazy removal)
    drv.set_now(101)
    drv.begin_compute([0], [40])
    drv.set_output([0], transient=[1])
    assert _entry(drv, 0) == (40, 104, AUTO) and drv.seen["overwrites"] == 1
    assert drv.tick(103)[1] == 3 and drv.tick(104)[1] == 1 and drv.tick(107)[1] == 2
    assert not drv.entries
    return drv


def scn_no_defaults(make):
    """No defaults: a handle without a code of its own stores nothing; a delay set back to 0 neither."""
    drv = make(slot_arrays(4), 0)
    drv.open()
    drv.auto_open()
    drv.set_auto_delay([1, 2], [4, 4], [0, 9])
    drv.set_auto_delay([2], [0])
    drv.begin_compute([0, 1, 2, 3], [5, 6, 7, 8])
    drv.set_output([0, 1, 2, 3], transient=[0, 0, 0, 1])
    assert {h: t for h, (_, t) in drv.entries.items()} == {1: 4}
    drv.begin_compute([2], [9])
    drv.set_output([2], transient=[1])
    assert _entry(drv, 2) == (9, 9, AUTO)
    return drv


def scn_ioso_delay(make):
    """Slot 1: Computing with has_delay, delay 50, auto 2, reached by a cascade (gains InvalidateOnSetOutput), then
    set_output: it survives its own cascade as Consistent + DelayStarted and gets its delay entry only."""
    drv = make(slot_arrays(3, consistent=[0], computing_delayed=[1], edges=[(0, 1)]), 0, now=10)
    drv.open()
    drv.auto_open()
    drv.set_delay([1], [50])
    drv.set_auto_delay([1], [2])
    assert list(drv.invalidate([0])) == [0]
    assert drv.states()[1][1] == COMPUTING | F_IOSO | F_HD and not drv.entries
    drv.set_output([1])
    assert drv.states()[1][1] == CONSISTENT | F_DS | F_HD
    v = int(drv.states()[0][1])
    assert drv.entries == {1: (v, 60)} and drv.kind[1] == 0 and drv.seen["ioso"] == 1
    assert drv.ca == dict(armed_auto=0, merged=0, fired_auto=0)
    assert drv.tick(12)[1] == 0
    ids, fired = drv.tick(60)
    assert list(ids) == [1] and fired == 1
    return drv


def scn_merge(make):
    """Both directions of AddOrUpdateToEarlier. X (slot 1): auto due 100, then a cascade at now = 10 with delay 3 ->
    due 13, kind auto. Y (slot 3): auto due 12, delay 50 -> stays 12; tick(12) invalidates it with DelayStarted set."""
    drv = make(slot_arrays(6, consistent=[0, 2]), 0)
    drv.open()
    drv.auto_open()
    drv.set_auto_delay([1, 3], [100, 12])
    drv.set_delay([1, 3], [3, 50])
    drv.begin_compute([1, 3], [31, 33], [1, 1])
    drv.add_used([1, 3], [0, 2])
    drv.set_output([1, 3])
    assert _entry(drv, 1) == (31, 100, AUTO) and _entry(drv, 3) == (33, 12, AUTO)
    drv.set_now(10)
    assert list(drv.invalidate([0])) == [0]
    assert _entry(drv, 1) == (31, 13, AUTO) and drv.ca["merged"] == 1
    assert list(drv.invalidate([2])) == [2]
    assert _entry(drv, 3) == (33, 12, AUTO) and drv.ca["merged"] == 2
    assert drv.c["armed"] == 2 and drv.c["dropped"] == 0
    drv.start_auto([1])                                  # auto on auto: min again (110 against 13)
    assert _entry(drv, 1) == (31, 13, AUTO) and drv.ca["merged"] == 3
    ids, fired = drv.tick(12)
    assert list(ids) == [3] and fired == 1 and (drv.states()[1][1] & F_DS)
    ids, fired = drv.tick(13)
    assert list(ids) == [1] and fired == 1
    assert drv.ca == dict(armed_auto=2, merged=3, fired_auto=2)
    return drv


def scn_delay_then_auto(make):
    """The other order: a delay entry first (kind 0, due 30), then start_auto with auto 4: due 4, kind auto."""
    drv = make(slot_arrays(3, consistent=[0], delayed=[1], edges=[(0, 1)]), 0)
    drv.open()
    drv.auto_open()
    drv.set_delay([1], [30])
    drv.set_auto_delay([1], [4])
    drv.invalidate([0])
    v = int(drv.states()[0][1])
    assert _entry(drv, 1) == (v, 30, 0)
    drv.start_auto([1])
    assert _entry(drv, 1) == (v, 4, AUTO) and drv.ca == dict(armed_auto=0, merged=1, fired_auto=0)
    assert drv.tick(4)[1] == 1
    return drv


def scn_displacement(make):
    """X (slot 1, delayed, delay 4) and Z (slot 2, no delay), both with auto entries due 20, displaced at now 3.
    X survives: its entry moves to the detached handle, kind kept, and the delay arm behind it brings the due
    time to 7. Z does not: nothing reaches a detached handle, its stale entry leaves at its due time."""
    drv = make(slot_arrays(4), 2)
    drv.open()
    drv.auto_open()
    drv.set_auto_delay([1, 2], [20, 20], [6, 6])
    drv.set_delay([1], [4])
    drv.begin_compute([1, 2], [51, 52], [1, 0])
    drv.set_output([1, 2])
    assert _entry(drv, 1) == (51, 20, AUTO) and _entry(drv, 2) == (52, 20, AUTO)
    drv.set_now(3)
    moved = drv.begin_compute([1, 2], [61, 62])
    assert len(moved) == 1
    d = moved[0]
    assert _entry(drv, d) == (51, 7, AUTO) and drv.c["moved"] == 1 and drv.ca["merged"] == 1
    assert set(drv.entries) == {d, 2} and drv.entries[2][0] == 52
    assert drv.adelay[d] == 20 and drv.tdelay[d] == 6    # the codes went with the node
    ids, fired = drv.tick(7)
    assert list(ids) == [d] and fired == 1
    dropped = drv.c["dropped"]
    assert drv.tick(20)[1] == 0 and drv.c["dropped"] == dropped + 1 and not drv.entries
    return drv


def scn_batch(make):
    """Three batches. (1) set_output then begin_compute on the same slots: slot 1's node (delayed) survives to a
    detached handle and is armed there with slot 1's delays, slot 2's does not and gets nothing. (2) set_output then
    invalidate of the same node: no entry. (3) two set_output steps of slots 4 and 5 with a recomputation between:
    slot 4's first node is gone, slot 5's (delayed) lives on detached; both second nodes are armed at their slots."""
    drv = make(slot_arrays(8), 4, default_transient=2)
    drv.open()
    drv.auto_open()
    drv.set_auto_delay([1, 2, 3, 4, 5], [9, 9, 9, 9, 9])
    drv.set_delay([1, 5], [30, 30])
    drv.begin_compute([1, 2, 3, 4, 5], [71, 72, 73, 74, 75], [1, 0, 0, 0, 1])
    drv.set_now(1)
    drv.batch([("set_output", [1, 2]), ("begin_compute", [1, 2], [81, 82])])
    (d1, e1), = drv.entries.items()
    assert d1 >= drv.n and e1 == (71, 10) and drv.kind[d1] == AUTO
    assert drv.ca == dict(armed_auto=1, merged=1, fired_auto=0)      # the move's delay arm: 31 against 10
    assert drv.seen["resolved_detached"] == 1 and drv.seen["resolved_none"] == 1
    drv.batch([("set_output", [3]), ("invalidate", [3])])
    assert list(drv.entries) == [d1] and drv.seen["not_consistent"] == 1
    drv.set_now(2)
    drv.batch([("set_output", [4, 5], [0, 1]), ("begin_compute", [4, 5], [84, 85], [0, 1]), ("set_output", [4, 5])])
    d5 = max(drv.entries)
    assert d5 >= drv.n and d5 != d1
    assert {h: _entry(drv, h) for h in drv.entries if h != d1} == {
        4: (84, 11, AUTO), 5: (85, 11, AUTO), d5: (75, 4, AUTO)}     # d5: transient (2), merged with its delay (32)
    assert drv.seen["resolved_detached"] == 2 and drv.seen["resolved_none"] == 2
    assert drv.tick(4)[1] == 1 and drv.tick(10)[1] == 1 and drv.tick(11)[1] == 2
    assert not drv.entries
    return drv


def scn_cascading(make):
    """A (slot 0, auto 5) is used by B (slot 1, delayed, delay 4): A's fired timer's wave flags B, which arms at
    now = 5 and fires at 9."""
    drv = make(slot_arrays(3), 0)
    drv.open()
    drv.auto_open()
    drv.set_auto_delay([0], [5])
    drv.set_delay([1], [4])
    drv.begin_compute([0], [91])
    drv.set_output([0])
    drv.begin_compute([1], [92], [1])
    drv.add_used([1], [0])
    drv.set_output([1])
    assert list(drv.entries) == [0]
    ids, fired = drv.tick(5)
    assert list(ids) == [0] and fired == 1
    assert _entry(drv, 1) == (92, 9, 0)
    assert drv.tick(8)[1] == 0
    ids, fired = drv.tick(9)
    assert list(ids) == [1] and fired == 1
    assert drv.ca == dict(armed_auto=1, merged=0, fired_auto=1)
    return drv


def scn_start_auto(make):
    """test_gpu_flagged.py's _mixed() graph (Consistent, Computing, Invalidated, empty, delayed and started nodes),
    registered in bulk: start_auto over every slot, every third one transient. Only Consistent nodes gain
    entries; the started ones, armed by open, merge."""
    arrays, waves, _ = _mixed()
    drv = make(arrays, MIXED_DET, default_delay=5, default_auto=6, default_transient=2)
    drv.open()
    started = len(drv.entries)
    assert started >= 3
    drv.auto_open()
    hs = np.arange(drv.n, dtype=np.uint32)
    odd = hs[1::2]
    drv.set_auto_delay(odd[:400], np.where(np.arange(400) % 4 == 0, NEVER, 3).astype(np.uint64))
    drv.start_auto(hs, (hs % 3 == 0).astype(np.uint8))
    f = arrays[1]
    consistent = int(np.sum((arrays[0] != 0) & ((f & 3) == CONSISTENT)))
    # (a started node that is also a never-coded candidate keeps its delay entry)
    assert consistent - drv.seen["auto_none"] <= len(drv.entries) <= consistent
    assert drv.ca["merged"] >= 3 and drv.seen["not_consistent"] >= 100 and 1 <= drv.seen["auto_none"] <= 100
    drv.invalidate(waves[0][0], waves[0][1])
    assert drv.tick(2)[1] >= 100
    assert drv.tick(3)[1] >= 50
    drv.start_auto(odd[:64])                             # again, on entries that fired and on some that did not
    drv.tick(6)
    drv.tick(20)
    assert not drv.entries
    return drv


GRID_N = 262_144 + 37


@functools.lru_cache(maxsize=None)
def _grid_arrays():
    """GRID_N Consistent nodes registered in bulk, then as many empty slots (computed once, read-only)."""
    n = 2 * GRID_N
    versions = np.zeros(n, np.uint64)
    versions[:GRID_N] = O.version_of(43, np.arange(GRID_N, dtype=np.uint64))
    flags = np.zeros(n, np.uint32)
    flags[:GRID_N] = CONSISTENT
    none = np.zeros(0, np.uint32)
    arrays = (versions, flags, none, none, np.zeros(0, np.uint64))
    for a in arrays:
        a.setflags(write=False)
    return arrays


def scn_past_one_grid(make):
    """start_auto over 262,181 Consistent handles and set_output of as many freshly begun slots (k_tm_arm_auto
    strides past its grid of at most 1,024 x 256 lanes, the last wavefront partial), every fifth transient
    (due 2, the others 6); tick(2) and tick(6) fire them all."""
    arrays = _grid_arrays()
    drv = make(arrays, 0, default_auto=6, default_transient=2)
    drv.open()
    drv.auto_open()
    a = np.arange(GRID_N, dtype=np.uint32)
    b = a + np.uint32(GRID_N)
    tr = (a % 5 == 0).astype(np.uint8)
    drv.start_auto(a, tr)
    assert len(drv.entries) == GRID_N
    drv.begin_compute(b, b.astype(np.uint64) + np.uint64(7))
    drv.set_output(b, transient=tr)
    assert len(drv.entries) == 2 * GRID_N
    n_tr = int(tr.sum())
    assert drv.tick(1)[1] == 0
    ids, fired = drv.tick(2)
    assert fired == 2 * n_tr and np.array_equal(ids, np.concatenate([a[tr == 1], b[tr == 1]]))
    ids, fired = drv.tick(6)
    assert fired == 2 * (GRID_N - n_tr) and not drv.entries
    return drv


def scn_computed_options(make, rounds=3):
    """AnonymousComputedTest.ComputedOptionsTest (:38-60) with the tick firing: a source (slot 0) with
    AutoInvalidationDelay = 2 ticks and a reader (slot 1) observing it. Each new output schedules its
    invalidation; a firing invalidates the source (and, the first time, the reader); a tick with nothing due is a
    no-op; the next Use() computes a new value. Returns (driver, values computed)."""
    drv = make(slot_arrays(2), 0)
    drv.open()
    drv.auto_open()
    drv.set_auto_delay([0], [2])
    values = 0

    def use():
        nonlocal values
        st = drv.states()
        if st[0][0] == 0 or (st[1][0] & 3) != CONSISTENT:
            values += 1
            drv.begin_compute([0], [100 + values])
            drv.set_output([0])
        return values

    assert use() == 1 and use() == 1
    drv.begin_compute([1], [200])
    drv.add_used([1], [0])
    drv.set_output([1])
    now = 0
    for k in range(rounds):
        assert drv.tick(now + 1)[1] == 0
        now += 2
        ids, fired = drv.tick(now)
        assert fired == 1 and list(ids) == ([0, 1] if k == 0 else [0])
        assert drv.tick(now)[1] == 0                     # a second firing finds nothing
        assert use() == k + 2
    assert use() > rounds
    assert (drv.states()[1][1] & 3) == INVALIDATED
    return drv, values


def _alone(arrays, n_det, **kw):
    return AutoDriver(arrays, n_det, **kw)


# ---- the model alone ---------------------------------------------------------------------------------------

def _identity(drv):
    c = drv.c
    assert c["armed"] == c["fired"] + c["dropped"] + len(drv.entries), c


def test_chain_model():
    drv = scn_chain(_alone)
    assert drv.c == dict(armed=1, fired=1, dropped=0, moved=0, runs=1)
    assert drv.ca == dict(armed_auto=1, merged=0, fired_auto=1) and drv.seen["fired_without_ds"] == 1


def test_selection_model():
    drv = scn_selection(_alone)
    assert drv.seen["overwrites"] >= 1 and drv.seen["unset"] == 8 and drv.seen["stale"] == 0
    assert drv.ca == dict(armed_auto=7, merged=0, fired_auto=6)
    _identity(drv)
    _identity(scn_no_defaults(_alone))


def test_ioso_and_merge_models():
    assert scn_ioso_delay(_alone).seen["ioso"] == 1
    a, b = scn_merge(_alone), scn_delay_then_auto(_alone)
    assert a.ca["merged"] + b.ca["merged"] >= 2 and a.ca["merged"] >= 2
    _identity(a)
    _identity(b)


def test_displacement_model():
    drv = scn_displacement(_alone)
    assert drv.c["moved"] == 1 and drv.seen["stale"] == 1 and drv.ca["fired_auto"] == 1
    _identity(drv)


def test_batch_model():
    drv = scn_batch(_alone)
    assert drv.seen["resolved_detached"] == 2 and drv.seen["resolved_none"] == 2 and drv.seen["not_consistent"] == 1
    assert drv.ca == dict(armed_auto=4, merged=2, fired_auto=4)
    _identity(drv)


def test_cascading_and_computed_options_models():
    scn_cascading(_alone)
    drv, values = scn_computed_options(_alone)
    assert values == 4 and drv.ca["fired_auto"] == 3


def test_start_auto_model():
    drv = scn_start_auto(_alone)
    assert drv.ca["merged"] >= 3 and drv.ca["fired_auto"] >= 1000, drv.ca
    assert drv.seen["not_consistent"] >= 100 and drv.seen["stale"] >= 1
    _identity(drv)


def test_past_one_grid_model():
    drv = scn_past_one_grid(_alone)
    assert GRID_N > M.GRID_LANES and GRID_N % 64 != 0            # k_tm_arm_auto's second trip, a partial last wavefront
    assert drv.n == 2 * GRID_N and 520_000 < drv.n < 530_000
    assert [t[1:] for t in drv.trace if t[0] == "start_auto"] == [(GRID_N,)]
    assert (GRID_N,) in [t[1:] for t in drv.trace if t[0] == "set_output"]
    ticks = [t[1:] for t in drv.trace if t[0] == "tick"]
    assert ticks[0] == (2 * GRID_N, 0) and ticks[1][1] == 2 * 52_437 and ticks[2] == (2 * (GRID_N - 52_437), 2 * (GRID_N - 52_437))
    assert all(t[0] > M.GRID_LANES for t in ticks)               # the due pass strides too
    assert drv.ca == dict(armed_auto=2 * GRID_N, merged=0, fired_auto=2 * GRID_N)
    _identity(drv)
