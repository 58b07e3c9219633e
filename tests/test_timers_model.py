"""The delay timers' semantics (fgi.h, C-ABI 0.11) as a small Python model over the CPU oracle, and the
scenarios test_gpu_timers.py drives the engine through. This file runs the model alone (no GPU) and checks that
the scenarios are not vacuous: a changed generator must not let the GPU cases pass on nothing.

The model (`Driver`) keeps a dict handle -> (version, due). After every oracle call it computes the flagged set
as the difference of two state dumps (`expected_flagged` of test_gpu_flagged.py), applies the arm and move rules
of fgi.h to the dict, and on a tick fires its due entries with `immediately` = 1. With an engine attached
(test_gpu_timers.py) every step is made on both and compared: the returned id set, the state dump over every
handle, fgi_timers_list, the fired count and the statistics. Expected values never come from the engine; the
one thing the model takes from it is which detached handle a displaced node was given (alone, it numbers them
itself)."""
import functools

import numpy as np

import fgo as O
from harness import COMPUTING, CONSISTENT, F_DS, F_HD, INVALIDATED
from test_gpu_flagged import N as MIXED_N, N_DET as MIXED_DET, _dump_handles, _mixed, expected_flagged

NEVER = 0xFFFFFFFFFFFFFFFF
NONE = 0xFFFFFFFF


def _u32(a):
    return np.asarray(a, np.uint32).reshape(-1)


class Driver:
    def __init__(self, arrays, n_det, default_delay=0, now=0, engine=None, fgi=None):
        versions, flags, src, dst, tags = arrays
        self.n, self.n_det = len(versions), n_det
        self.o = O.Oracle(self.n)
        self.o.load_graph(versions, flags, src, dst, tags)
        self.g, self.fgi = engine, fgi
        self.det = {}                      # detached handle -> oracle node
        self.free = list(range(self.n + n_det - 1, self.n - 1, -1))   # the model's own numbering (no engine)
        self.delay, self.entries = {}, {}
        self.now, self.default = now, default_delay
        self.c = dict(armed=0, fired=0, dropped=0, moved=0, runs=0)
        self.seen = dict(never=0, overwrites=0, stale=0, displaced_armed=0)
        # what the steps were made of, for the model-alone tests: ("wave", nodes flagged), ("tick", entries stored
        # going in, entries fired), ("move", pairs of one displacement), ("release", entries dropped), and what a
        # scenario adds itself
        self.trace = []

    # ---- the rules of fgi.h ----
    def states(self):
        return _dump_handles(self.o, self.n, self.n_det, self.det)

    def _waiting(self, st, h):
        v, f = st
        return v[h] != 0 and (f[h] & 3) == CONSISTENT and (f[h] & F_DS) != 0

    def _arm(self, h, st):
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
        e = self.entries.get(h)
        if e is not None and e[0] == v:
            return False               # the earlier due time stays
        if e is not None:
            self.c["dropped"] += 1
            self.seen["overwrites"] += 1
        self.entries[h] = (v, min(self.now + d, NEVER - 1))
        self.c["armed"] += 1
        return True

    def _move(self, s, d, st):
        s, d = int(s), int(d)
        if s in self.delay:
            self.delay[d] = self.delay[s]
        else:
            self.delay.pop(d, None)
        e = self.entries.get(s)
        if e is not None and st[0][d] != 0 and e[0] == int(st[0][d]):
            self.entries[d] = self.entries.pop(s)
            self.c["moved"] += 1
        elif self._arm(d, st):
            self.seen["displaced_armed"] += 1

    @staticmethod
    def _invalidated(before, after):
        (bv, bf), (av, af) = before, after
        return np.nonzero((bv != 0) & ((bf & 3) != INVALIDATED) & ((af & 3) == INVALIDATED) & (av == bv))[0].astype(np.uint32)

    def _oracle_wave(self, roots, imm):
        roots = _u32(roots)
        imm = np.zeros(len(roots), np.uint8) if imm is None else np.asarray(imm, np.uint8)
        slot = roots < self.n
        if slot.any():
            self.o.invalidate_slots(roots[slot], imm[slot])
        if (~slot).any():
            self.o.invalidate_nodes([self.det[int(h)] for h in roots[~slot]], imm[~slot])

    # ---- steps, each made on the oracle + model and, with an engine, on the engine too ----
    def open(self):
        if self.g:
            self.g.timers_open(self.default, self.now)
        st = self.states()
        for h in range(self.n + self.n_det):
            self._arm(h, st)
        self.check()

    def set_delay(self, handles, delays):
        for h, d in zip(_u32(handles), np.asarray(delays, np.uint64)):
            if int(d):
                self.delay[int(h)] = int(d)
            else:
                self.delay.pop(int(h), None)
        if self.g:
            self.g.timers_set_delay(handles, delays)

    def set_now(self, now):
        self.now = now
        if self.g:
            self.g.timers_set_now(now)

    def invalidate(self, roots, imm=None, how="sync", direction=None):
        before = self.states()
        self._oracle_wave(roots, imm)
        after = self.states()
        flagged = expected_flagged(before, after)[0]
        for h in flagged:
            self._arm(h, after)
        self.trace.append(("wave", len(flagged)))
        want = self._invalidated(before, after)
        if self.g:
            if direction is not None:
                self.g.set_option(self.fgi.OPT_DIRECTION, direction)
            if how == "async":
                got = self.g.wave_wait_ids(self.g.invalidate_async_host(_u32(roots), imm))
            else:
                got = self.g.invalidate(_u32(roots), imm)
            assert np.array_equal(np.sort(got), want), f"invalidated sets differ: {len(got)} vs {len(want)}"
        self.check()
        return want

    def tick(self, now):
        """fgi_timers_run_due(now): (ids of the fired timers' wave, entries fired)."""
        assert now >= self.now
        self.now = now
        st = self.states()
        due = sorted(h for h, (_, t) in self.entries.items() if t <= now)
        stored = len(self.entries)
        fire = []
        for h in due:
            v, _ = self.entries.pop(h)
            if self._waiting(st, h) and int(st[0][h]) == v:
                fire.append(h)
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
            if fire:
                assert np.array_equal(self.g.last_wave_ids(), want)
        self.check()
        return want, len(fire)

    def _oracle_begin(self, slots, versions, has_delay, handles):
        """begin_compute on the oracle; handles: the engine's detached handles or None. Returns the (slot,
        detached handle) pairs of the displaced nodes that live on, and the slots whose node the call invalidated:
        by the displacement itself, or before it by the cascade of an earlier item of the same call (the oracle
        takes the items one by one; such a node is no longer registered when its slot's turn comes)."""
        moves = []
        bv, bf = self.states()
        for i, (s, v) in enumerate(zip(_u32(slots), np.asarray(versions, np.uint64))):
            _, displaced = self.o.begin_compute(int(s), int(v), bool(has_delay[i]) if has_delay is not None else False)
            lives = displaced != O.NONE and (self.o.node_info(displaced)[2] & 3) != INVALIDATED
            if handles is not None:
                assert (handles[i] != NONE) == lives, f"slot {s}: detached handle {handles[i]}, the oracle's node lives: {lives}"
            if lives:
                d = int(handles[i]) if handles is not None else self.free.pop()
                assert d not in self.det, f"detached handle {d} handed out while it still names a node"
                self.det[d] = displaced
                moves.append((int(s), d))
        moved = {s for s, _ in moves}
        inv = [int(s) for s in _u32(slots) if bv[s] != 0 and (bf[s] & 3) != INVALIDATED and int(s) not in moved]
        return moves, inv

    def begin_compute(self, slots, versions, has_delay=None):
        handles = self.g.begin_compute(_u32(slots), versions, has_delay) if self.g else None
        before = self.states()
        moves, _ = self._oracle_begin(slots, versions, has_delay, handles)
        after = self.states()
        for h in expected_flagged(before, after)[0]:   # the displacement cascade's
            self._arm(h, after)
        for s, d in moves:
            self._move(s, d, after)
        self.trace.append(("move", len(moves)))
        self.check()
        return [d for _, d in moves]

    def _node(self, h):
        return self.o.last(int(h)) if h < self.n else self.det[int(h)]

    def set_output(self, handles):
        before = self.states()
        for h in _u32(handles):
            self.o.set_output(self._node(h))
        after = self.states()
        for h in expected_flagged(before, after)[0]:
            self._arm(h, after)
        if self.g:
            self.g.set_output(_u32(handles))
        self.check()

    def add_used(self, dependants, used):
        for d, u in zip(_u32(dependants), _u32(used)):
            self.o.add_used(self._node(d), self._node(u))
        if self.g:
            self.g.add_used(_u32(dependants), _u32(used))
        self.check()

    def release(self, handles):
        dropped = self.c["dropped"]
        for h in _u32(handles):
            del self.det[int(h)]
            self.free.append(int(h))
            if self.entries.pop(int(h), None) is not None:
                self.c["dropped"] += 1
        self.trace.append(("release", self.c["dropped"] - dropped))
        if self.g:
            self.g.release(_u32(handles))
        self.check()

    def batch(self, steps):
        """fgi_run_batch: the steps on the oracle one by one; behind them the moves in step order, then the arm
        rule once over everything the cascades flagged, on the states the batch left."""
        outs = None
        if self.g:
            got, outs = self.g.run_batch(steps)
        cand, moves, want = [], [], []
        for k, sp in enumerate(steps):
            before = self.states()
            step_inv = []
            if sp[0] == "invalidate":
                self._oracle_wave(sp[1], sp[2] if len(sp) > 2 else None)
            elif sp[0] == "begin_compute":
                m, step_inv = self._oracle_begin(sp[1], sp[2], sp[3] if len(sp) > 3 else None,
                                                 outs[k] if outs is not None else None)
                moves += m
            elif sp[0] == "add_used":
                for d, u in zip(_u32(sp[1]), _u32(sp[2])):
                    self.o.add_used(self._node(d), self._node(u))
                continue
            elif sp[0] == "set_output":
                for h in _u32(sp[1]):
                    self.o.set_output(self._node(h))
            after = self.states()
            cand += list(expected_flagged(before, after)[0])
            want.append(np.sort(np.append(self._invalidated(before, after), step_inv).astype(np.uint32)))
        st = self.states()
        for s, d in moves:
            self._move(s, d, st)
        for h in cand:
            self._arm(h, st)
        want = np.concatenate(want).astype(np.uint32) if want else np.zeros(0, np.uint32)
        if self.g:
            assert np.array_equal(got, want), f"the batch's ids: {len(got)} vs {len(want)}"
        self.check()
        return want

    # ---- the engine against the model ----
    def listed(self):
        hs = sorted(self.entries)
        return (np.array(hs, np.uint32), np.array([self.entries[h][0] for h in hs], np.uint64),
                np.array([self.entries[h][1] for h in hs], np.uint64))

    def check(self):
        if not self.g:
            return
        gv, gf = self.g.dump_states()
        ov, of = self.states()
        assert np.array_equal(gv, ov), f"versions differ at {np.nonzero(gv != ov)[0][:8]}"
        bad = np.nonzero(gf != of)[0]
        assert len(bad) == 0, f"state_flags differ at {bad[:8]}: engine {gf[bad[:8]]} oracle {of[bad[:8]]}"
        h, v, d = self.g.timers_list()
        mh, mv, md = self.listed()
        assert np.array_equal(h, mh), f"stored handles: engine {len(h)}, model {len(mh)}; {np.setxor1d(h, mh)[:8]}"
        assert np.array_equal(v, mv), "stored versions differ"
        assert np.array_equal(d, md), f"due times differ at handles {h[np.nonzero(d != md)[0][:8]]}"
        st = self.g.timers_stats()
        assert st["armed"] == st["fired"] + st["dropped"] + st["stored"], st
        assert st["stored"] == len(self.entries), (st, len(self.entries))
        for k, want in self.c.items():
            assert st[k] == want, (k, st, self.c)
        due, stored = self.g.timers_next_due()
        assert due == (min(md) if len(md) else NEVER) and stored == len(self.entries)


def chain_arrays(n, edges, delayed=(), seed=3, computing=()):
    versions = O.version_of(seed, np.arange(n, dtype=np.uint64)).copy()
    flags = np.full(n, CONSISTENT, np.uint32)
    flags[list(delayed)] |= F_HD
    for c in computing:
        flags[c] = COMPUTING
    src = np.array([e[0] for e in edges], np.uint32)
    dst = np.array([e[1] for e in edges], np.uint32)
    return versions, flags, src, dst, versions[dst]


# ---- scenarios: make(arrays, n_det, **kw) -> Driver (with or without an engine) ------------------------------

def scn_chain(make):
    """a -> b -> c -> d (delay 5) -> e."""
    drv = make(chain_arrays(5, [(0, 1), (1, 2), (2, 3), (3, 4)], delayed=[3]), 0)
    drv.open()
    drv.set_delay([3], [5])
    assert list(drv.invalidate([0])) == [0, 1, 2]
    assert drv.entries == {3: (int(drv.states()[0][3]), 5)}
    runs = drv.c["runs"]
    ids, fired = drv.tick(4)
    assert len(ids) == 0 and fired == 0
    assert drv.c["runs"] == runs and min(t for _, t in drv.entries.values()) == 5
    ids, fired = drv.tick(5)
    assert list(ids) == [3, 4] and fired == 1 and not drv.entries
    return drv


@functools.lru_cache(maxsize=None)
def _mixed_plan():
    """What the mixed-states scenario draws besides _mixed()'s own graph and waves (computed once)."""
    arrays, waves, _ = _mixed()
    versions, flags = arrays[0], arrays[1]
    rng = np.random.default_rng(0x71AE)
    delayed = np.nonzero((versions != 0) & ((flags & F_HD) != 0))[0].astype(np.uint32)
    choice = np.array([1, 3, 7, 0, NEVER], np.uint64)
    delays = choice[rng.integers(0, len(choice), len(delayed))]
    wide = rng.choice(MIXED_N, 600, replace=False).astype(np.uint32)
    return delayed, delays, wide


def scn_mixed(make, directions=(1, 2, 0)):
    """test_gpu_flagged.py's _mixed() graph (4,096 slots, 64 detached handles; Computing, delayed, already
    started and stale nodes), delays drawn from {1, 3, 7, default (5), never}; its three waves (push, pull, auto)
    interleaved with ticks, a displacement of stored and of never-flagged delayed nodes, a slot reused under a
    stored entry and flagged again (an overwrite by another version), and a wide fourth wave."""
    arrays, waves, _ = _mixed()
    delayed, delays, wide = _mixed_plan()
    drv = make(arrays, MIXED_DET, default_delay=5)
    drv.open()                         # arms what the graph holds already started, with the default delay
    drv.set_delay(delayed, delays)
    drv.invalidate(waves[0][0], waves[0][1], direction=directions[0])
    drv.tick(2)
    # displaced: stored nodes (their entries move) and delayed nodes no wave reached yet (armed by the call)
    st = drv.states()
    stored = [h for h in sorted(drv.entries) if h < drv.n][:6]
    fresh = [int(h) for h in delayed if int(h) not in drv.entries and (st[1][h] & 3) == CONSISTENT
             and not (st[1][h] & F_DS) and drv.delay.get(int(h), 0) != NEVER][:6]
    slots = np.array(stored + fresh, np.uint32)
    drv.begin_compute(slots, st[0][slots] + np.uint64(1000), np.ones(len(slots), np.uint8))
    drv.set_output(slots)
    # a slot reused under a stored entry: invalidated at once, computed again, hung under a root, flagged again
    reuse = np.array([h for h in sorted(drv.entries) if h < drv.n and drv.entries[h][1] > 4][:4], np.uint32)
    assert len(reuse) >= 1
    drv.invalidate(reuse, np.ones(len(reuse), np.uint8))
    hub = next(h for h in range(drv.n) if (drv.states()[1][h] & 0x1F) == CONSISTENT and h not in drv.entries)
    v = drv.states()[0]
    drv.begin_compute(reuse, v[reuse] + np.uint64(2000), np.ones(len(reuse), np.uint8))
    drv.add_used(reuse, np.full(len(reuse), hub, np.uint32))
    drv.set_output(reuse)
    drv.invalidate(waves[1][0], waves[1][1], direction=directions[1])
    drv.tick(4)
    drv.invalidate([hub], direction=directions[2])
    drv.invalidate(waves[2][0], waves[2][1], direction=directions[2])
    drv.tick(9)
    drv.invalidate(wide, direction=directions[0])
    drv.tick(12)
    drv.tick(40)
    return drv


def scn_edges(make):
    """Entries at handles 0, 63, 64, n - 1 and at both detached handles; a tick with 70 due entries; a tick with
    600 due entries scattered among 1,400 that stay."""
    n, n_det = 2048, 2
    edges = [(1, h) for h in range(n) if h != 1]
    drv = make(chain_arrays(n, edges, delayed=[h for h in range(n) if h != 1], seed=9), n_det)
    drv.open()
    hs = np.array([h for h in range(n) if h != 1], np.uint32)
    first = np.array([0, 63, 64] + list(range(130, 197)), np.uint32)          # 70
    second = np.array([h for h in hs if h % 3 == 0 and h not in set(first.tolist())][:600], np.uint32)
    delays = np.full(n, 100, np.uint64)
    delays[first] = 2
    delays[second] = 4
    drv.set_delay(hs, delays[hs])
    assert list(drv.invalidate([1])) == [1]
    assert len(drv.entries) == n - 1
    moved = drv.begin_compute([2, n - 2], drv.states()[0][[2, n - 2]] + np.uint64(10))
    assert sorted(moved) == [n, n + 1] and drv.c["moved"] == 2
    assert {0, 63, 64, n - 1, n, n + 1} <= set(drv.entries)
    assert drv.tick(2)[1] == 70
    assert drv.tick(4)[1] == 600 and len(drv.entries) == n - 1 - 670
    assert drv.tick(100)[1] == n - 1 - 670 and not drv.entries
    return drv


def scn_slot_reuse(make):
    drv = make(chain_arrays(4, [(0, 1)], delayed=[1], seed=4), 2)
    drv.open()
    drv.set_delay([1], [5])
    drv.invalidate([0])
    assert list(drv.entries) == [1]
    drv.set_now(1)
    assert list(drv.invalidate([1], [1])) == [1]          # X goes before its due time; its entry stays
    assert list(drv.entries) == [1]
    assert drv.begin_compute([1], [drv.states()[0][1] + np.uint64(2)], [1]) == []
    drv.set_output([1])
    dropped = drv.c["dropped"]
    ids, fired = drv.tick(6)
    assert len(ids) == 0 and fired == 0
    assert drv.c["dropped"] == dropped + 1 and not drv.entries
    assert drv.states()[1][1] == CONSISTENT | F_HD        # Y is untouched
    return drv


def scn_displacement(make):
    """Slot 1: X, stored at now 0 (due 5), displaced at now 2. Slot 2: W, delayed, never flagged, displaced by
    the same call. Slots 3 / 4 depend on X / W."""
    drv = make(chain_arrays(8, [(0, 1), (1, 3), (2, 4)], delayed=[1, 2], seed=6), 4)
    drv.open()
    drv.set_delay([1, 2], [5, 5])
    drv.invalidate([0])
    xv = int(drv.states()[0][1])
    assert drv.entries == {1: (xv, 5)}
    drv.set_now(2)
    d1, d2 = drv.begin_compute([1, 2], drv.states()[0][[1, 2]] + np.uint64(2))
    assert drv.entries[d1] == (xv, 5) and drv.entries[d2][1] == 7 and set(drv.entries) == {d1, d2}
    assert drv.c["moved"] == 1
    ids, fired = drv.tick(5)
    assert fired == 1 and sorted(ids) == [3, d1]          # X under its detached handle, and its row's dependant
    st = drv.states()
    assert (st[1][1] & 3) == COMPUTING and (st[1][2] & 3) == COMPUTING   # the slots' new nodes are untouched
    dropped = drv.c["dropped"]
    drv.release([d2])
    assert drv.c["dropped"] == dropped + 1 and not drv.entries
    assert drv.tick(7)[1] == 0
    return drv


def scn_cascading(make):
    """0 -> 1 (delay 3) -> 2 (delay 4) -> 3: the first timer's wave starts the second."""
    drv = make(chain_arrays(4, [(0, 1), (1, 2), (2, 3)], delayed=[1, 2], seed=8), 0)
    drv.open()
    drv.set_delay([1, 2], [3, 4])
    drv.invalidate([0])
    assert [t for _, t in drv.entries.values()] == [3]
    ids, fired = drv.tick(3)
    assert list(ids) == [1] and fired == 1
    assert {h: t for h, (_, t) in drv.entries.items()} == {2: 7}
    assert drv.tick(6)[1] == 0
    ids, fired = drv.tick(7)
    assert list(ids) == [2, 3] and fired == 1
    return drv


def scn_batch(make):
    """The streaming schedule at 64 hubs x 40 leaves, every 8th leaf delayed (delays 5, 15, 25 in turn): four
    rounds of one batch each (recompute last round's hubs and all their leaves, hang the leaves under the hubs,
    a wave over four hubs), each followed by a tick 5 later. The leaves whose timers have not fired yet are
    displaced with stored entries."""
    H, L = 64, 40
    n = H + H * L
    leaf = np.arange(H, n, dtype=np.uint32)
    hub_of = lambda ls: ((np.asarray(ls, np.int64) - H) // L).astype(np.uint32)
    delayed = leaf[(leaf - H) % L % 8 == 7]
    versions = O.version_of(12, np.arange(n, dtype=np.uint64)).copy()
    flags = np.full(n, CONSISTENT, np.uint32)
    flags[delayed] |= F_HD
    has_delay = np.zeros(n, np.uint8)
    has_delay[delayed] = 1
    drv = make((versions, flags, hub_of(leaf), leaf, versions[leaf]), 256)
    drv.open()
    drv.set_delay(delayed, np.array([5, 15, 25], np.uint64)[np.arange(len(delayed)) % 3])
    prev = np.zeros(0, np.uint32)
    moved_total = 0
    for r in range(4):
        drv.set_now(10 * r)
        roots = np.arange(4 * r, 4 * r + 4, dtype=np.uint32)
        ls = (H + prev.astype(np.int64)[:, None] * L + np.arange(L)[None, :]).ravel().astype(np.uint32)
        v = drv.states()[0]
        steps = []
        if len(prev):
            with_entry = [int(s) for s in ls if int(s) in drv.entries]
            assert len(with_entry) >= 4, "no BEGIN_COMPUTE on a slot that holds a stored entry"
            steps += [("begin_compute", prev, v[prev] + np.uint64(2)), ("set_output", prev),
                      ("begin_compute", ls, v[ls] + np.uint64(2), has_delay[ls]), ("add_used", ls, hub_of(ls)),
                      ("set_output", ls)]
        steps.append(("invalidate", roots))
        before = drv.c["moved"]
        drv.batch(steps)
        moved_total += drv.c["moved"] - before
        assert drv.tick(10 * r + 5)[1] >= 1
        prev = roots
    assert moved_total >= 8
    drv.tick(200)
    assert not drv.entries
    return drv


def scn_async(make):
    arrays, waves, _ = _mixed()
    drv = make(arrays, MIXED_DET, default_delay=3)
    drv.open()
    stored = len(drv.entries)
    drv.invalidate(waves[0][0], waves[0][1], how="async")
    assert len(drv.entries) > stored + 10               # the ticket's wave armed its entries
    assert drv.tick(3)[1] > 10
    return drv


def scn_open_populated(make):
    arrays, _, _ = _mixed()
    drv = make(arrays, MIXED_DET, default_delay=5, now=100)
    drv.open()
    started = np.nonzero(((arrays[1] & 3) == CONSISTENT) & ((arrays[1] & F_DS) != 0) & (arrays[0] != 0))[0]
    assert len(started) >= 3 and sorted(drv.entries) == list(started)
    assert all(t == 105 for _, t in drv.entries.values())
    assert drv.tick(105)[1] == len(started)
    return drv


def hub_arrays(sizes, seed, started=()):
    """One hub per entry of sizes (handles 0 .. len(sizes) - 1), hub k -> sizes[k] leaves, hub after hub; every
    leaf has an InvalidationDelay, the listed ones DelayStarted already. Returns (arrays, the hubs' leaves)."""
    H, n = len(sizes), len(sizes) + int(sum(sizes))
    versions = O.version_of(seed, np.arange(n, dtype=np.uint64)).copy()
    flags = np.full(n, CONSISTENT, np.uint32)
    flags[H:] |= F_HD
    flags[np.asarray(started, np.int64)] |= F_DS
    leaf = np.arange(H, n, dtype=np.uint32)
    src = np.repeat(np.arange(H, dtype=np.uint32), sizes)
    bounds = H + np.concatenate([[0], np.cumsum(sizes)])
    return (versions, flags, src, leaf, versions[leaf]), [leaf[a - H:b - H] for a, b in zip(bounds[:-1], bounds[1:])]


GRID_A, GRID_B, GRID_DET = 280_000, 4_096 + 37, 64


@functools.lru_cache(maxsize=None)
def _grid_plan():
    """scn_past_one_grid's graph and delays (computed once, read-only afterwards): the arrays, the leaves of
    hub 0 and of hub 1, the leaves already started, the delay of every leaf, and the one leaf with delay 1."""
    n = 2 + GRID_A + GRID_B
    a0 = np.arange(2, 2 + GRID_A, dtype=np.uint32)
    started = np.concatenate([a0[::131][:2000], np.arange(n - 37, n, dtype=np.uint32)])
    arrays, (A, B) = hub_arrays([GRID_A, GRID_B], 31, started)
    leaves = np.concatenate([A, B])
    delays = np.full(len(leaves), 100, np.uint64)
    for r, d in ((3, 2), (7, 4), (11, 0), (13, NEVER)):
        delays[leaves % 50 == r] = d
    one = int(B[5])
    delays[one - 2] = 1
    assert len(started) == 2037 and one not in set(started.tolist())
    for a in arrays + (A, B, started, leaves, delays):
        a.setflags(write=False)
    return arrays, A, B, started, leaves, delays, one


def scn_past_one_grid(make, until=None):
    """Two hubs over 280,000 and 4,133 leaves, every leaf delayed, default delay 7: every grid-stride loop of
    the timer kernels makes a second trip (the arm kernel over every handle at open and over 278,000 records, the
    due pass over more than 262,144 entries three times, the min-reduction over more than 65,536), the last
    wavefront of the last trip is partial, and ticks fire more than 4,096 entries. until: stop after that many
    ticks."""
    arrays, A, B, started, leaves, delays, one = _grid_plan()
    drv = make(arrays, GRID_DET, default_delay=7)
    drv.open()                         # 2,000 started leaves spread over A and the last 37 handles of the graph
    assert sorted(drv.entries) == sorted(started.tolist())
    drv.set_delay(leaves, delays)
    assert list(drv.invalidate([0])) == [0]
    before = len(drv.entries)
    assert one not in drv.entries
    assert list(drv.invalidate([1])) == [1]
    # the unique smallest due time belongs to an entry armed behind `before` others (nothing has left the pool)
    assert [h for h, (_, t) in drv.entries.items() if t == 1] == [one] and min(t for _, t in drv.entries.values()) == 1
    drv.trace.append(("min_after", before))
    ticks = 0
    for now in (1, 2, 4, 7, 100):
        if until is not None and ticks == until:
            return drv
        if now == 4:   # entries of nodes that go before their due time: stale when they come due (at 4, 7, 100)
            stale = np.array(sorted(drv.entries)[::90][:3000], np.uint32)
            assert len(stale) == 3000
            assert np.array_equal(drv.invalidate(stale, np.ones(len(stale), np.uint8)), stale)
        drv.tick(now)
        ticks += 1
    assert not drv.entries
    return drv


def scn_pool_growth(make):
    """Hub 0 -> 900 leaves A, hub 1 -> 3,000 leaves B, 512 detached handles, no default delay: the pool grows
    while it holds 600 entries, the fired list is reallocated behind it, the delay table passes 64 delays, two
    displacements of 300 and 150 stored nodes around a release of 150 detached handles with entries."""
    arrays, (A, B) = hub_arrays([900, 3000], 33)
    drv = make(arrays, 512)
    drv.open()
    drv.set_delay(A, np.where(np.arange(len(A)) % 3 == 0, 3, 50).astype(np.uint64))
    drv.invalidate([0])
    assert len(drv.entries) == 900
    assert drv.tick(3)[1] == 300
    drv.trace.append(("delays", len(set(drv.delay.values())), len(drv.entries)))
    drv.set_delay(B, (20 + np.arange(len(B)) % 200).astype(np.uint64))
    drv.trace.append(("delays", len(set(drv.delay.values())), len(drv.entries)))
    drv.invalidate([1])
    assert len(drv.entries) == 3600
    held = np.array(sorted(drv.entries), np.uint32)
    first = np.concatenate([held[held < B[0]][:100], held[held >= B[0]][:200]])
    v = drv.states()[0]
    d1 = drv.begin_compute(first, v[first] + np.uint64(10), np.ones(len(first), np.uint8))
    assert len(d1) == 300 and drv.c["moved"] == 300
    drv.release(d1[::2])
    assert drv.c["dropped"] == 150 and len(drv.entries) == 3450
    second = held[held >= B[0]][200:350]
    d2 = drv.begin_compute(second, v[second] + np.uint64(10), np.ones(len(second), np.uint8))
    assert len(d2) == 150 and drv.c["moved"] == 450
    assert len(set(d2) & set(d1[::2])) >= 100      # released handles handed out again
    assert drv.tick(30)[1] >= 100 and len(drv.entries) >= 3000
    drv.tick(400)
    assert not drv.entries
    return drv


def scn_delay_churn(make):
    """Delay codes pass from the leaves of hub 0 to those of hub 1 while the first ones' entries are still
    stored: the pool holds the old entries and the new ones together."""
    arrays, (A, B) = hub_arrays([2000, 2000], 35)
    drv = make(arrays, 0)
    drv.open()
    drv.set_delay(A, np.full(len(A), 5, np.uint64))
    drv.invalidate([0])
    drv.set_delay(A, np.zeros(len(A), np.uint64))      # by fgi.h the entries stay
    assert len(drv.entries) == 2000
    drv.set_delay(B, np.full(len(B), 5, np.uint64))
    drv.set_now(1)
    drv.invalidate([1])
    drv.trace.append(("churn", len(drv.entries), len(A)))
    assert drv.tick(5)[1] == 2000
    assert drv.tick(6)[1] == 2000
    return drv


def scn_saturation(make):
    """scn_chain's graph at now = 2^64 - 10: a + b -> c -> d (delay 100: now + delay wraps), f (never) and
    g (delay 9: now + delay == FGI_TIMER_NEVER) hang off c. Both due times are FGI_TIMER_NEVER - 1."""
    now = 2**64 - 10
    drv = make(chain_arrays(7, [(0, 1), (1, 2), (2, 3), (3, 4), (2, 5), (2, 6)], delayed=[3, 5, 6]), 0, now=now)
    drv.open()
    drv.set_delay([3, 5, 6], [100, NEVER, 9])
    assert list(drv.invalidate([0])) == [0, 1, 2]
    v = drv.states()[0]
    assert drv.entries == {3: (int(v[3]), NEVER - 1), 6: (int(v[6]), NEVER - 1)} and drv.seen["never"] == 1
    ids, fired = drv.tick(NEVER - 2)
    assert len(ids) == 0 and fired == 0 and len(drv.entries) == 2
    ids, fired = drv.tick(NEVER - 1)
    assert list(ids) == [3, 4, 6] and fired == 2 and not drv.entries
    return drv


def scn_begin_reaches_own_slots(make):
    """0 -> 1 -> 2, and one BEGIN_COMPUTE step over all three slots: the displacement of 0 invalidates the nodes of
    1 and 2 before their own turn comes (the oracle finds no registered node to displace there). The step's ids
    are all three slots, whichever item invalidated them."""
    drv = make(chain_arrays(4, [(0, 1), (1, 2)], seed=5), 2)
    drv.open()
    v = drv.states()[0]
    ids = drv.batch([("begin_compute", [0, 1, 2], v[[0, 1, 2]] + np.uint64(2))])
    assert list(ids) == [0, 1, 2] and not drv.det
    assert list(drv.batch([("begin_compute", [3], v[[3]] + np.uint64(2)), ("invalidate", [0, 3])])) == [3]
    return drv


def scn_displaced_and_reached(make):
    """0 -> 1 (delayed, delay 5, never flagged), and one fgi_begin_compute over both slots: the displacement of 0
    reaches 1 along the edge, and 1 is displaced by the same call. Its node has no entry when the call begins, so
    it is armed under its detached handle (no move), exactly as the delayed node of slot 2, which no edge reaches."""
    drv = make(chain_arrays(4, [(0, 1)], delayed=[1, 2], seed=7), 3)
    drv.open()
    drv.set_delay([1, 2], [5, 5])
    drv.set_now(2)
    v = drv.states()[0]
    d1, d2 = drv.begin_compute([0, 1, 2], v[[0, 1, 2]] + np.uint64(2))
    assert drv.entries == {d1: (int(v[1]), 7), d2: (int(v[2]), 7)}
    assert drv.c == dict(armed=2, fired=0, dropped=0, moved=0, runs=0) and drv.seen["displaced_armed"] == 2
    assert drv.tick(7)[1] == 2
    return drv


def _alone(arrays, n_det, **kw):
    return Driver(arrays, n_det, **kw)


# ---- the model alone ---------------------------------------------------------------------------------------

def test_chain_model():
    drv = scn_chain(_alone)
    assert drv.c == dict(armed=1, fired=1, dropped=0, moved=0, runs=1)


def test_mixed_model_is_not_vacuous():
    drv = scn_mixed(_alone)
    c, s = drv.c, drv.seen
    assert c["fired"] >= 50, c
    assert s["stale"] >= 1 and c["moved"] >= 1 and s["overwrites"] >= 1 and s["never"] >= 1, (c, s)
    assert s["displaced_armed"] >= 1, s
    assert c["armed"] == c["fired"] + c["dropped"] + len(drv.entries)


def test_edges_model():
    drv = scn_edges(_alone)
    assert drv.c["fired"] == 2047 and drv.c["runs"] == 3


def test_small_scenarios_model():
    assert scn_slot_reuse(_alone).seen["stale"] == 1
    d = scn_displacement(_alone)
    assert d.c["moved"] == 1 and d.seen["displaced_armed"] == 1
    assert scn_cascading(_alone).c == dict(armed=2, fired=2, dropped=0, moved=0, runs=2)


def test_displaced_and_reached_model():
    assert scn_displaced_and_reached(_alone).c == dict(armed=2, fired=2, dropped=0, moved=0, runs=1)


def test_begin_reaches_own_slots_model():
    drv = scn_begin_reaches_own_slots(_alone)
    assert (drv.states()[1][:4] & 3).tolist() == [COMPUTING] * 4


def test_batch_model():
    drv = scn_batch(_alone)
    assert drv.c["moved"] >= 8 and drv.c["fired"] >= 20
    assert drv.c["armed"] == drv.c["fired"] + drv.c["dropped"]


def test_async_and_open_model():
    scn_async(_alone)
    scn_open_populated(_alone)


# ---- the large scenarios against the sizes timers.hip's kernels and buffers are written for -------------------
GRID_LANES = 1024 * 256    # tgrid(): at most 1,024 blocks of kTBlock = 256 lanes; k_tm_arm and k_tm_due stride past it
MIN_THREADS = 1 << 16      # fgi_timers_next_due launches k_tm_min over at most 2^16 threads
IMM_FIRST = 4096           # fgi_timers_run_due: the fired roots' flags (imm) start at 4,096 bytes
DTAB_FIRST = 64            # fgi_timers_set_delay: the delay table (dtab) starts at 64 delays
POOL_FIRST = 1024          # tm_reserve: the pool's smallest capacity
MOVE_BLOCK = 256           # timers_move launches k_tm_move with kTBlock = 256 pairs per block


def _traced(drv, kind):
    return [t[1:] for t in drv.trace if t[0] == kind]


def test_past_one_grid_model():
    drv = scn_past_one_grid(_alone)
    _, A, B, started, leaves, delays, one = _grid_plan()
    assert drv.n + drv.n_det > GRID_LANES and (drv.n + drv.n_det) % 64 != 0      # the pass over every handle at open
    assert started.max() >= GRID_LANES and started.max() == drv.n - 1
    waves, ticks = _traced(drv, "wave"), _traced(drv, "tick")
    assert waves[0][0] == 278_000 and waves[0][0] > GRID_LANES                   # records of one arm launch
    assert waves[1][0] == len(B) - 37 == 4096
    assert [t[0] for t in ticks[:2]] == [278_491, 278_490]
    assert sum(t[0] > GRID_LANES for t in ticks) >= 2, ticks                     # due passes with a second trip
    assert [t[0] > GRID_LANES for t in ticks] == [True, True, True, True, False], ticks
    assert any(t[0] > GRID_LANES and t[0] % 64 != 0 for t in ticks)              # ... whose last wavefront is partial
    assert ticks[0][1] == 1 and ticks[1][1] == 5642
    assert sum(t[1] > IMM_FIRST for t in ticks) >= 2, ticks
    assert _traced(drv, "min_after")[0][0] > MIN_THREADS
    assert drv.seen["stale"] == 3000 and drv.seen["never"] >= 5000
    assert drv.c["armed"] == drv.c["fired"] + drv.c["dropped"] == 278_491 and drv.c["runs"] == 5
    # what test_gpu_timers.py's capacity case expects of tick(2), from the plan alone
    short = scn_past_one_grid(_alone, until=1)
    want, fired = short.tick(2)
    assert fired == 5642 and np.array_equal(want, grid_tick2_ids())


def grid_tick2_ids():
    """The handles scn_past_one_grid's tick(2) invalidates: the leaves with delay 2 that the waves started."""
    _, _, _, started, leaves, delays, _ = _grid_plan()
    return np.setdiff1d(leaves[delays == 2], started).astype(np.uint32)


def test_pool_growth_model():
    drv = scn_pool_growth(_alone)
    (d0, held0), (d1, held1) = _traced(drv, "delays")
    assert d0 <= DTAB_FIRST < d1 and d1 == 201                 # the table is regrown by the second set_delay
    assert held0 == held1 == 600                               # ... and so is the pool, holding entries:
    assert POOL_FIRST < held1 + len(drv.delay) + drv.n_det     # the bound passes the capacity the pool has then
    moves = [m[0] for m in _traced(drv, "move")]
    assert moves == [300, 150] and moves[0] > MOVE_BLOCK
    assert _traced(drv, "release") == [(150,)] and 150 >= 100  # tombstones going into the next due pass
    ticks = _traced(drv, "tick")
    assert ticks[0] == (900, 300)
    assert ticks[1][0] == 3450 and ticks[1][0] + 150 > 2 * POOL_FIRST   # the pool passed the fired list made at tick(3)
    assert drv.c == dict(armed=3900, fired=3750, dropped=150, moved=450, runs=3)


def test_delay_churn_model():
    drv = scn_delay_churn(_alone)
    (stored, a), = _traced(drv, "churn")
    # A bound of "the most delay codes there ever were" (|A|) gives a pool of max(|A|, 2 * 1,024) records: the
    # pool starts at 1,024 and grows to the larger of the bound and its double. The scenario stores more than
    # that, and reaches twice the larger of |A| and 1,024 (with 2 x 2,000 leaves it equals it: 4,000).
    assert stored == 4000 and stored > max(a, 2 * POOL_FIRST) and stored >= 2 * max(a, POOL_FIRST)
    assert drv.c == dict(armed=4000, fired=4000, dropped=0, moved=0, runs=2)


def test_saturation_model():
    drv = scn_saturation(_alone)
    assert drv.c == dict(armed=2, fired=2, dropped=0, moved=0, runs=1)
