"""A seeded random walk over the timers' models with the fan-out table and the state view added: the generator
test_gpu_walk.py drives the engine with, and the combined model (`FullDriver`) it is compared against. A helper
module: test_walk_model.py runs it alone (no GPU) and checks that the walks are not vacuous.

`FullDriver` is test_auto_timers_model.py's `AutoDriver` (delay and auto timers over the CPU oracle) plus
  * the subscription table of fgi.h's replica fan-out as a dict handle -> [(peer, call id)]: fgi_subscribe stores
    nothing on an empty or Invalidated handle, the same triple twice is two entries, the fan-out that delivers an
    entry removes it, entries move with the node (`_move`; a batch moves them behind itself in step order),
    fgi_release and fgi_unsubscribe_peer drop and count them. After every call that ran cascades the driver takes the
    fan-out (fgi_last_wave_fanout after a wave, a mutation or a tick that fired; fgi_fanout_ids over the ascending
    union of a batch's ids or over an asynchronous ticket's ids) and compares it with the model's join. Taking it
    every time also keeps fgi.h's host rule: no entry is left on an invalidated slot when a computation begins there.
    A tick that fired nothing must leave fgi_last_wave_fanout's answer as it was;
  * the state view: `planes_from_flags` of the model's dump over every handle, compared in check() while a view is open;
  * layers that open late: until open() the model arms nothing and check() reads no timer call;
  * prune / prune_range on engine and oracle, which may change nothing check() compares.
Expected values never come from the engine; the one thing the model takes from it is which detached handle a
displaced node was given.

`walk` draws every operation from the model's own state (never from the engine), through the step interface that
`Driver`, `AutoDriver` and `PartDriver` share, so a partition takes it with a smaller `ops`.

fgi_restore is left out of the walk: fgi.h leaves the subscription table alone while the detached-handle list
reverts to the snapshot's, so an entry on a reverted detached handle has no defined owner."""
import collections
import functools
import hashlib

import numpy as np

from harness import COMPUTING, CONSISTENT, F_DS, F_HD, INVALIDATED, random_states
from test_gpu_flagged import _edges_from_live, expected_flagged
import test_auto_timers_model as A
from test_auto_timers_model import AUTO
from test_timers_model import NEVER, NONE, _u32

N_PEERS = 7
ROUTES = ("last", "batch", "ticket")


def _join(items, n_peers):
    """(peer, handle, call) triples -> (peer_off, call_ids, handles) by peer, handle, call id (test_gpu_fanout.py's
    np_join order)."""
    items = sorted(items)
    off = np.zeros(n_peers + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(np.array([p for p, _, _ in items], np.int64), minlength=n_peers))
    return off, np.array([c for _, _, c in items], np.uint64), np.array([h for _, h, _ in items], np.uint32)


class FullDriver(A.AutoDriver):
    def __init__(self, arrays, n_det, n_peers=N_PEERS, **kw):
        super().__init__(arrays, n_det, **kw)
        self.n_peers = n_peers
        self.timers_on = False
        self.subs = {}                     # handle -> [(peer, call id)]
        self.sc = dict(stored=0, delivered=0, dropped=0)
        self.routes = dict.fromkeys(ROUTES, 0)
        self.seen.update(resolved_detached=0, resolved_none=0, sub_invalidated=0, subs_moved=0, subs_released=0,
                         subs_unsubscribed=0, reused_after_drop=0)
        self.view = None
        self.tainted = set()               # released detached handles whose release dropped an entry or a subscription
        self.delivered = hashlib.sha256()  # every fan-out the model made, in order
        self._hold = 0
        self._dead = []
        self._fan = None

    # ---- layers that may open late ----
    def open(self):
        self.timers_on = True
        super().open()

    def open_view(self):
        if self.g:
            self.view = self.g.open_state_view()
        self.check()

    def _arm(self, h, st):
        return super()._arm(h, st) if self.timers_on else False

    # ---- the fan-out table ----
    @property
    def live(self):
        return sum(len(v) for v in self.subs.values())

    def _move_subs(self, s, d):
        moved = self.subs.pop(s, None)
        if moved:
            self.subs[d] = moved
            self.seen["subs_moved"] += len(moved)

    def _move(self, s, d, st):
        s, d = int(s), int(d)
        assert d not in self.subs, f"detached handle {d} handed out while the model holds subscriptions on it"
        self._move_subs(s, d)
        if self.timers_on:
            super()._move(s, d, st)

    def _take(self, h):
        """The entries a fan-out delivers for invalidated handle h: they leave the table."""
        return self.subs.pop(h, [])

    def _deliver(self, inv, route):
        items = [(p, int(h), c) for h in inv for p, c in self._take(int(h))]
        self.sc["delivered"] += len(items)
        self.routes[route] += len(items)
        self.delivered.update(repr((route, sorted(items))).encode())
        return _join(items, self.n_peers)

    def _engine_fan(self):
        """fgi_last_wave_fanout as it answers now: the canonical arrays, or the status it refuses with."""
        from test_gpu_fanout import canon
        try:
            return tuple(a.tolist() for a in canon(*self.g.last_wave_fanout(self.n_peers)))
        except Exception as e:             # FgiError: after a batch or an asynchronous ticket
            return ("status", getattr(e, "status", repr(e)))

    def _fanout(self, inv, route):
        want = self._deliver(inv, route)
        if self.g:
            from test_gpu_fanout import assert_fanout
            if route == "last":
                got = self.g.last_wave_fanout(self.n_peers)
            else:
                got = self.g.fanout_ids(np.asarray(inv, np.uint32), self.n_peers)
            assert_fanout(got, want, f"the fan-out ({route}) of {len(inv)} ids")

    def subscribe(self, handles, peers, calls):
        st = self.states()
        want = []
        for h, p, c in zip(_u32(handles), _u32(peers), np.asarray(calls, np.uint64)):
            h = int(h)
            dead = st[0][h] == 0 or (st[1][h] & 3) == INVALIDATED
            want.append(int(dead))
            if dead:
                self.seen["sub_invalidated"] += 1
            else:
                self.subs.setdefault(h, []).append((int(p), int(c)))
                self.sc["stored"] += 1
        if self.g:
            got = self.g.subscribe(_u32(handles), _u32(peers), np.asarray(calls, np.uint64))
            assert list(got) == want, f"fgi_subscribe's results differ at {np.nonzero(got != np.array(want))[0][:8]}"
        self.check()
        return want

    def unsubscribe_peer(self, peer):
        n = 0
        for h in list(self.subs):
            keep = [e for e in self.subs[h] if e[0] != peer]
            n += len(self.subs[h]) - len(keep)
            if keep:
                self.subs[h] = keep
            else:
                del self.subs[h]
        self.sc["dropped"] += n
        self.seen["subs_unsubscribed"] += n
        if self.g:
            got = self.g.unsubscribe_peer(int(peer))
            assert got == n, f"fgi_unsubscribe_peer({peer}) dropped {got}, the model {n}"
        self.check()
        return n

    # ---- steps with their fan-out ----
    def _held(self, fn, *a, **kw):
        self._hold += 1
        try:
            return fn(*a, **kw)
        finally:
            self._hold -= 1

    def invalidate(self, roots, imm=None, how="sync", direction=None):
        want = self._held(super().invalidate, roots, imm, how=how, direction=direction)
        self._fanout(want, "ticket" if how == "async" else "last")
        self.check()
        return want

    def _oracle_begin(self, slots, versions, has_delay, handles):
        moves, inv = super()._oracle_begin(slots, versions, has_delay, handles)
        for _, d in moves:
            if d in self.tainted:
                self.tainted.discard(d)
                self.seen["reused_after_drop"] += 1
        self._dead = inv
        return moves, inv

    def begin_compute(self, slots, versions, has_delay=None):
        before = self.states()
        out = self._held(super().begin_compute, slots, versions, has_delay)
        inv = np.union1d(self._invalidated(before, self.states()), np.array(self._dead, np.uint32)).astype(np.uint32)
        if self.g:
            got = self.g.last_wave_ids()
            assert np.array_equal(got, inv), f"the displacement cascade's ids: engine {got.tolist()}, model {inv.tolist()}"
        self._fanout(inv, "last")
        self.check()
        return out

    def set_output(self, handles, transient=None):
        before = self.states()
        self._held(super().set_output, handles, transient)
        inv = self._invalidated(before, self.states())
        if self.g:
            got = self.g.last_wave_ids()
            assert np.array_equal(got, inv), f"fgi_set_output's cascade ids: engine {got.tolist()}, model {inv.tolist()}"
        self._fanout(inv, "last")
        self.check()

    def _drop_entry(self, h):
        if self.entries.pop(h, None) is not None:
            self.c["dropped"] += 1
            return True
        return False

    def release(self, handles):
        dropped = self.c["dropped"]
        for h in _u32(handles):
            h = int(h)
            del self.det[h]
            self.free.append(h)
            gone = self.subs.pop(h, [])
            self.sc["dropped"] += len(gone)
            self.seen["subs_released"] += len(gone)
            if self._drop_entry(h) or gone:
                self.tainted.add(h)
        self.trace.append(("release", self.c["dropped"] - dropped))
        if self.g:
            self.g.release(_u32(handles))
        self.check()

    def _fires(self, st, h, v, auto):
        live = st[0][h] != 0 and (st[1][h] & 3) == CONSISTENT and int(st[0][h]) == v
        return bool(live and (auto or (st[1][h] & F_DS)))

    def tick(self, now):
        """AutoDriver.tick with the fan-out behind a tick that fired, and fgi_last_wave_fanout's answer kept by one
        that did not."""
        assert now >= self.now
        self.now = now
        st = self.states()
        due = sorted(h for h, (_, t) in self.entries.items() if t <= now)
        stored = len(self.entries)
        fire = []
        for h in due:
            v, _ = self.entries.pop(h)
            auto = self.kind[h] & AUTO
            if self._fires(st, h, v, auto):
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
            stood = None if fire else self._engine_fan()
            self.g.fire = np.array(fire, np.uint32)          # for an engine pair: the roots of the tick's wave
            got, fired = self.g.timers_run_due(now)
            assert fired == len(fire), f"fired {fired}, the model {len(fire)}"
            assert np.array_equal(got, want), f"the fired timers' wave: {len(got)} ids vs {len(want)}"
            if fire:
                assert np.array_equal(self.g.last_wave_ids(), want)
            else:
                assert self._engine_fan() == stood, "a tick that fired nothing changed fgi_last_wave_fanout's answer"
        if fire:
            self._fanout(want, "last")
        self.check()
        return want, len(fire)

    def _resolve(self, cand, h):
        return cand

    def _batch_ops(self, ops, cands, st):
        for i, op in enumerate(ops):
            if op[0] == "begin":
                for s, d in op[2].items():
                    self._move(s, d, st)
            elif self.auto:
                for h, c, t, cand in zip(op[1], op[2], op[3], cands[i]):
                    if c == 1:
                        cand = self._resolve(cand, int(h))
                        self.seen["resolved_detached"] += int(cand not in (NONE, int(h)))
                        self.seen["resolved_none"] += int(cand == NONE)
                        self._auto_arm(cand, h, t, st)

    def _after_batch(self, ops, cands, flagged, st):
        self._batch_ops(ops, cands, st)
        for h in flagged:
            self._arm(h, st)

    def batch(self, steps):
        """AutoDriver.batch (the same walk over the steps) with the fan-out over the ascending union of its ids."""
        outs = None
        if self.g:
            got, outs = self.g.run_batch(steps)
        flagged, ops, want = [], [], []
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
        self._after_batch(ops, cands, flagged, st)
        want = np.concatenate(want).astype(np.uint32) if want else np.zeros(0, np.uint32)
        if self.g:
            assert np.array_equal(got, want), f"the batch's ids: engine {got.tolist()}, model {want.tolist()}"
        self._fanout(np.unique(want), "batch")
        self.check()
        return want

    def prune_range(self, lo, count):
        self.o.prune_range(int(lo), int(count))
        if self.g:
            self.g.prune_range(int(lo), int(count))
        self.check()

    def prune(self):
        self.o.prune()
        if self.g:
            self.g.prune()
        self.check()

    # ---- the engine against the model ----
    def check(self):
        if self._hold or not self.g:
            return
        ov, of = self.states()
        if self.timers_on:
            super().check()
        else:
            gv, gf = self.g.dump_states()
            assert np.array_equal(gv, ov), f"versions differ at {np.nonzero(gv != ov)[0][:8]}"
            bad = np.nonzero(gf != of)[0]
            assert len(bad) == 0, f"state_flags differ at {bad[:8]}: engine {gf[bad[:8]]} oracle {of[bad[:8]]}"
        st = self.g.sub_stats()
        want = dict(live=self.live, delivered=self.sc["delivered"], dropped=self.sc["dropped"])
        assert {k: st[k] for k in want} == want, (st, want)
        assert st["delivered"] + st["dropped"] + st["live"] == self.sc["stored"], (st, self.sc)
        if self.view is not None:
            from test_gpu_state_view import assert_view
            assert_view(self.view, ov, of, "the state view")

    def fingerprint(self):
        """Everything check() compares, and every fan-out made, as one comparable value."""
        h, v, d = self.listed()
        sv, sf = self.states()
        return (h.tolist(), v.tolist(), d.tolist(), self.kinds().tolist(), dict(self.c), dict(self.ca), dict(self.sc),
                self.live, self.delivered.hexdigest(), hashlib.sha256(sv.tobytes() + sf.tobytes()).hexdigest())


# ---- the graph ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walk_arrays(seed, n, m):
    """random_states(p_delay=0.2) over n slots with m edges out of its Consistent nodes (read-only)."""
    rng = np.random.default_rng(seed)
    versions, flags = random_states(n, rng, p_delay=0.2)
    arrays = (versions, flags) + _edges_from_live(versions, flags, rng, m, n)
    for a in arrays:
        a.setflags(write=False)
    return arrays


def draw_defaults(seed):
    """The graph defaults of a seed, each from {0, small}: (default_delay, default_auto, default_transient)."""
    rng = np.random.default_rng(seed ^ 0xDEFA)
    return tuple(int(x) for x in rng.choice([0, 5], 3))


# ---- the generator -----------------------------------------------------------------------------------------
ALL_OPS = ("wave", "wave_async", "compute", "batch", "tick", "release", "set_stray", "start_auto", "subscribe",
           "unsubscribe", "prune", "overwrite")
PART_OPS = ("wave", "compute", "batch", "tick", "release")
WEIGHTS = dict(wave=12, wave_async=6, compute=16, batch=14, tick=18, release=5, set_stray=4, start_auto=5,
               subscribe=9, unsubscribe=2, prune=4, overwrite=5)
DELAYS = np.array([0, 3, 6, 12, NEVER], np.uint64)
LAYERS = ("timers", "auto", "subs", "view")


class Skip(Exception):
    """An operation's precondition does not hold: the walk replaces it."""


class _Gen:
    def __init__(self, drv, rng):
        self.drv, self.rng = drv, rng
        self.full = isinstance(drv, FullDriver)
        self.vnext = (1 << 55) + 1      # odd, above every version_of value, within the engine's 56 bits
        self.call = 1000
        self.subs_on = False

    # ---- what the model holds ----
    # Detached handles are always listed in the order they were handed out (drv.det's own order), never by number:
    # which number a displaced node gets is the engine's choice, and the walk must not depend on it. The model alone
    # and the model with an engine attached then walk through the same operations on the same nodes.
    def _ordered(self, table):
        """The handles of `table` that name a node: slots ascending, then detached handles as handed out."""
        drv = self.drv
        return [h for h in sorted(table) if h < drv.n] + [d for d in drv.det if d in table]

    def _spare(self):
        """The detached handles that name nothing, ascending."""
        drv = self.drv
        return [d for d in range(drv.n, drv.n + drv.n_det) if d not in drv.det]

    def _versions(self, k):
        v = self.vnext + 2 * np.arange(k, dtype=np.uint64)
        self.vnext += 2 * k
        return v.astype(np.uint64)

    def _room(self, slots):
        """Whether the detached handles the owners have free cover the nodes a BEGIN_COMPUTE on `slots` can displace."""
        drv = self.drv
        if hasattr(drv, "owner"):
            need = collections.Counter(drv.owner(s) for s in slots)
            held = collections.Counter(drv.owner(d) for d in drv.det)
            return all(held[r] + k <= drv.rank_det for r, k in need.items())
        return len(drv.det) + len(slots) <= drv.n_det

    def _roots(self, k):
        drv, rng = self.drv, self.rng
        pool = np.arange(drv.n, dtype=np.uint32)
        if self.full and drv.det:
            pool = np.concatenate([pool, np.array(list(drv.det), np.uint32)])
        roots = [int(x) for x in rng.choice(pool, min(k, len(pool)), replace=False)]
        held = self._ordered(getattr(drv, "subs", {}))
        for _ in range(max(1, k // 2)):    # up to half from the handles that hold subscriptions
            if held:
                roots.append(int(held[int(rng.integers(0, len(held)))]))
        roots = np.array(list(dict.fromkeys(roots)), np.uint32)
        return roots, (rng.random(len(roots)) < 0.3).astype(np.uint8)

    def _begin_slots(self, k):
        drv, rng = self.drv, self.rng
        slots = set(int(x) for x in rng.choice(drv.n, k, replace=False))
        # two of the slots that hold subscriptions and two that hold stored timer entries: what a displacement moves
        for table in (getattr(drv, "subs", {}), drv.entries):
            held = [h for h in sorted(table) if h < drv.n]
            for _ in range(2):
                if held:
                    slots.add(int(held[int(rng.integers(0, len(held)))]))
        return np.array(sorted(slots), np.uint32)

    def _compute_steps(self, k, second):
        drv, rng = self.drv, self.rng
        slots = self._begin_slots(k)
        hd = (rng.random(len(slots)) < 0.3).astype(np.uint8)
        # `used` names a node (fgi.h: an empty handle counts as Invalidated there; the oracle has no node to ask)
        nodes = np.setdiff1d(np.nonzero(drv.states()[0][:drv.n])[0], slots).astype(np.uint32)
        used = rng.choice(nodes, len(slots)).astype(np.uint32)
        done = slots[rng.random(len(slots)) < 0.8]
        tr = (rng.random(len(done)) < 0.3).astype(np.uint8)
        steps = [("begin_compute", slots, self._versions(len(slots)), hd), ("add_used", slots, used),
                 ("set_output", done, tr) if self.full else ("set_output", done)]
        again = done[::3] if second else done[:0]
        if not self._room(list(slots) + list(again)):
            raise Skip("no free detached handle")
        if len(again):
            steps.append(("begin_compute", again, self._versions(len(again)), np.ones(len(again), np.uint8)))
        return steps

    # ---- the operations: each returns the driver calls it is made of ----
    def wave(self, how="sync"):
        roots, imm = self._roots(int(self.rng.integers(1, 13)))
        kw = dict(direction=int(self.rng.integers(0, 3)))
        if how != "sync":
            kw["how"] = how
        return [("invalidate", (roots, imm), kw)]

    def wave_async(self):
        return self.wave("async")

    def compute(self):
        steps = self._compute_steps(int(self.rng.integers(4, 25)), False)
        return [(sp[0], sp[1:], {}) for sp in steps]

    def batch(self):
        roots, imm = self._roots(int(self.rng.integers(1, 7)))
        steps = [("invalidate", roots, imm)] + self._compute_steps(int(self.rng.integers(4, 17)), True)
        return [("batch", (steps,), {})]

    def tick(self):
        drv = self.drv
        if not getattr(drv, "timers_on", True):
            raise Skip("timers not open")
        calls = []
        now = drv.now
        if self.rng.random() < 0.3:
            now += 1
            calls.append(("set_now", (now,), {}))
        return calls + [("tick", (now + int(self.rng.integers(0, 3)),), {})]

    def release(self, every=False):
        drv = self.drv
        live = np.array(list(drv.det), np.uint32)
        if not len(live):
            raise Skip("no detached handle is held")
        pick = live if every else live[self.rng.random(len(live)) < 0.5]
        return [("release", (pick if len(pick) else live[:1],), {})]

    def set_stray(self):
        v, f = self.drv.states()
        stray = np.array(self._ordered(set(np.nonzero((v != 0) & ((f & 3) == COMPUTING))[0].tolist())), np.uint32)
        if not len(stray):
            raise Skip("no Computing node")
        hs = self.rng.choice(stray, min(len(stray), 12), replace=False).astype(np.uint32)
        return [("set_output", (hs, (self.rng.random(len(hs)) < 0.3).astype(np.uint8)), {})]

    def start_auto(self):
        drv = self.drv
        if not drv.auto:
            raise Skip("auto timers not open")
        pool = np.array(list(range(drv.n)) + list(drv.det) + self._spare(), np.uint32)
        hs = self.rng.choice(pool, 30, replace=False).astype(np.uint32)
        return [("start_auto", (hs, (self.rng.random(30) < 0.3).astype(np.uint8)), {})]

    def subscribe(self):
        drv, rng = self.drv, self.rng
        if not self.subs_on:
            raise Skip("no subscriptions yet")
        k = int(rng.integers(1, 41))
        live, spare = list(drv.det), self._spare()
        hs, ps, cs = [], [], []
        for _ in range(k):
            if hs and rng.random() < 0.15:             # the same triple again
                j = int(rng.integers(0, len(hs)))
                h, p, c = hs[j], ps[j], cs[j]
            else:
                u = rng.random()
                h = int(live[int(rng.integers(0, len(live)))]) if live and u < 0.25 else \
                    int(spare[int(rng.integers(0, len(spare)))]) if spare and u < 0.28 else int(rng.integers(0, drv.n))
                p, c = int(rng.integers(0, drv.n_peers)), self.call
                self.call += 1
            hs.append(h), ps.append(p), cs.append(c)
        return [("subscribe", (np.array(hs, np.uint32), np.array(ps, np.uint32), np.array(cs, np.uint64)), {})]

    def unsubscribe(self):
        if not self.subs_on:
            raise Skip("no subscriptions yet")
        return [("unsubscribe_peer", (int(self.rng.integers(0, self.drv.n_peers)),), {})]

    def prune(self):
        if self.rng.random() < 0.25:
            return [("prune", (), {})]
        lo = int(self.rng.integers(0, self.drv.n))
        return [("prune_range", (lo, int(self.rng.integers(1, self.drv.n - lo + 1))), {})]

    def overwrite(self):
        """scn_mixed's "slot reused under a stored entry": invalidated at once, begun with has_delay, hung under a
        Consistent hub, set, and flagged again through the hub: an entry of another version is overwritten."""
        drv = self.drv
        v, f = drv.states()
        held = [h for h in sorted(drv.entries) if h < drv.n and drv.entries[h][1] > drv.now + 1]
        hubs = np.nonzero((v[:drv.n] != 0) & ((f[:drv.n] & 0x1F) == CONSISTENT))[0]
        hubs = [int(h) for h in hubs if int(h) not in drv.entries]
        if not held or not hubs:
            raise Skip("no stored entry on a slot")
        s = held[int(self.rng.integers(0, len(held)))]
        hub = hubs[int(self.rng.integers(0, len(hubs)))]
        one = np.ones(1, np.uint8)
        return [("invalidate", ([s], one), {}), ("set_delay", ([s], [6]), {}),
                ("begin_compute", ([s], self._versions(1), one), {}), ("add_used", ([s], [hub]), {}),
                ("set_output", ([s],), {}), ("invalidate", ([hub],), {})]

    # ---- layers ----
    def layer(self, name):
        drv, rng = self.drv, self.rng
        half = np.sort(rng.choice(drv.n, drv.n // 2, replace=False)).astype(np.uint32)
        draw = lambda: DELAYS[rng.integers(0, len(DELAYS), len(half))]
        if name == "timers":
            return [("open", (), {}), ("set_delay", (half, draw()), {})]
        if name == "auto":
            return [("auto_open", (), {}), ("set_auto_delay", (half, draw(), draw()), {})]
        if name == "view":
            return [("open_view", (), {})]
        self.subs_on = True
        return self.subscribe()


def _show(x):
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (list, tuple)):
        return [_show(y) for y in x]
    return x


def walk(drv, rng, steps, ops=ALL_OPS, stop_at=None, layers=None, seed=None):
    """`steps` random operations on drv. layers: {step index: layer name} opened before that step's operation (default:
    every layer the driver has, before step 0). stop_at=k replays the first k steps. Returns the log (one entry per
    step: index, operation, the operation it replaces or None, the driver calls with their arguments) and the number
    of replaced operations. An assertion carries the seed, the step, the operation and its arguments."""
    gen = _Gen(drv, rng)
    if layers is None:
        layers = {-1: LAYERS if gen.full else ("timers",)}
    weights = np.array([WEIGHTS[o] for o in ops], float)
    weights /= weights.sum()
    log, replaced = [], 0

    def run(i, op, was, calls):
        log.append((i, op, was, [(name, _show(a), _show(sorted(kw.items()))) for name, a, kw in calls]))
        for name, a, kw in calls:
            try:
                getattr(drv, name)(*a, **kw)
            except AssertionError as e:
                raise AssertionError(f"seed {seed}, step {i}, {op}: {name}{tuple(_show(a))} {kw}: {e}") from e

    for i in sorted(k for k in layers if k < 0):
        for name in layers[i]:
            run(i, "open:" + name, None, gen.layer(name))
    for i in range(steps if stop_at is None else min(steps, stop_at)):
        for name in ([layers[i]] if isinstance(layers.get(i), str) else layers.get(i, ())):
            run(i, "open:" + name, None, gen.layer(name))
        op, was = str(ops[int(rng.choice(len(ops), p=weights))]), None
        try:
            calls = getattr(gen, op)()
        except Skip:
            # replaced, not dropped: a mutation that found no free detached handle releases them all, anything else
            # becomes a wave
            was, replaced = op, replaced + 1
            if op in ("compute", "batch") and drv.det:
                op, calls = "release", gen.release(every=True)
            else:
                op, calls = "wave", gen.wave()
        run(i, op, was, calls)
    return log, replaced


# ---- the walks of test_walk_model.py (model alone) and test_gpu_walk.py (engine attached): the same seeds and sizes --
SEEDS = (11, 23, 37)
N, N_DET, EDGES, STEPS = 1000, 90, 6000, 200            # 1,090 handles: a partial wavefront, a partial bitmap word
PART_N, PART_DET, PART_STEPS = 512, 40, 100


def counters(drv):
    """What a walk went through, whatever numbers its detached handles had."""
    return {k: dict(getattr(drv, k)) for k in ("c", "ca", "sc", "routes", "seen") if hasattr(drv, k)}, len(drv.entries)


def full_walk(make, seed, steps=STEPS, **kw):
    """The walk of `seed` over make(arrays, n_det, defaults...) -> FullDriver: (driver, log, replaced operations)."""
    dd, da, dt = draw_defaults(seed)
    drv = make(walk_arrays(seed, N, EDGES), N_DET, default_delay=dd, default_auto=da, default_transient=dt)
    log, replaced = walk(drv, np.random.default_rng(seed), steps, seed=seed, **kw)
    return drv, log, replaced


def late_layers(seed, steps=STEPS):
    """Each layer at a random step of the first half: timers before auto, the view last, subscriptions anywhere."""
    rng = np.random.default_rng(seed ^ 0x1A7E)
    at = np.sort(rng.integers(0, steps // 2, 4))
    first = [str(x) for x in rng.permutation(["timers", "auto", "subs"])]
    if first.index("timers") > first.index("auto"):
        i, j = first.index("timers"), first.index("auto")
        first[i], first[j] = first[j], first[i]
    layers = {}
    for k, name in zip(at, first + ["view"]):
        layers[int(k)] = layers.get(int(k), ()) + (name,)
    return layers


def part_walk(make, seed, steps=PART_STEPS):
    """The partition's walk: make(arrays, n_det per rank, default_delay) -> PartDriver. The default delay is always
    set: half the displaced nodes' entries fire under detached handles, which run no wave."""
    drv = make(walk_arrays(seed, PART_N, 3 * PART_N), PART_DET, default_delay=4)
    log, replaced = walk(drv, np.random.default_rng(seed), steps, ops=PART_OPS, seed=seed)
    return drv, log, replaced
