"""The delay timers per rank of a partition (fgi_part_timers_*, C-ABI 0.12) against the model of
test_part_timers_model.py.

The ranks are in-process groups on one GPU (`_build_with`). `Group` gives the model's `PartDriver` the Graph-like
calls over the group, in model handles (global slots, then every rank's detached handles): plain waves go
through fgi_part_local_invalidate, mutations through fgi_part_local_run_batch (one step per call, a batch whole),
ticks through fgi_part_local_timers_run_due. After every step the engine must equal the model in the invalidated
ids per rank (fgi_part_last_wave_ids: ascending, owned), fgi_dump_states of every rank, fgi_timers_list per rank,
the fired and detached counts per rank, fgi_timers_next_due and the summed counters. Expected values never come
from the engine; the one thing the model takes from it is which detached handle a displaced node was given.
The gates at the end check what the model does not cover."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_flagged import N as MIXED_N, _engine, _mixed
from test_gpu_part_host import _free_port
from test_gpu_part_state_view import _build_with, _each_rank
import test_part_timers_model as PM
import test_timers_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF


def to_model(n, block, n_det, r, local):
    """Rank r's local handles as model handles."""
    local = np.asarray(local, np.int64)
    return np.where(local < block, r * block + local, n + r * n_det + (local - block)).astype(np.uint32)


class Group:
    def __init__(self, pkg, gs, block, n, n_det):
        self.pkg, self.fgi, self.gs, self.block, self.n, self.n_det = pkg, pkg.fgi, gs, block, n, n_det
        self.P = len(gs)
        assert all(g.n_handles == block + n_det for g in gs)

    def _range(self, r):
        return r * self.block, min(self.n, (r + 1) * self.block)

    def _local(self, handles):
        """Model handles (detached ones) -> per rank local handles."""
        out = [[] for _ in self.gs]
        for h in M._u32(handles):
            assert h >= self.n, "a slot where a detached handle is expected"
            out[(int(h) - self.n) // self.n_det].append(self.block + (int(h) - self.n) % self.n_det)
        return out

    def close(self):
        for g in self.gs:
            g.close()

    # ---- the calls the Driver makes ----
    def timers_open(self, default_delay=0, now=0):
        for g in self.gs:
            g.part_timers_open(default_delay, now)

    def timers_set_delay(self, handles, delays):
        for g in self.gs:   # every rank is handed the whole list and keeps its share
            g.part_timers_set_delay(handles, delays)

    def timers_set_now(self, now):
        for g in self.gs:
            g.timers_set_now(now)

    def set_option(self, opt, value):
        for g in self.gs:
            g.set_option(opt, value)

    def _wave_ids(self, what):
        out = []
        for r, g in enumerate(self.gs):
            ids = g.part_last_wave_ids()
            lo, hi = self._range(r)
            assert np.all(np.diff(ids.astype(np.int64)) > 0), f"{what}, rank {r}: ids not strictly ascending"
            assert np.all((ids >= lo) & (ids < hi)), f"{what}, rank {r}: ids outside the rank's slots"
            out.append(ids)
        return out

    def invalidate(self, roots, imm=None):
        self.fgi.part_local_invalidate(self.gs, roots, imm)
        return np.concatenate(self._wave_ids("wave"))

    def _handles_out(self, slots, out):
        slots = M._u32(slots)
        return np.array([NONE if d == NONE else to_model(self.n, self.block, self.n_det, int(s) // self.block, [d])[0]
                         for s, d in zip(slots, out)], np.uint32)

    def begin_compute(self, slots, versions, has_delay=None):
        step = ("begin_compute", M._u32(slots), np.asarray(versions, np.uint64))
        if has_delay is not None:
            step += (np.asarray(has_delay, np.uint8),)
        _, outs, _ = self.fgi.part_local_run_batch(self.gs, [step])
        return self._handles_out(slots, outs[0])

    def set_output(self, handles):
        self.fgi.part_local_run_batch(self.gs, [("set_output", M._u32(handles))])

    def add_used(self, dependants, used):
        self.fgi.part_local_run_batch(self.gs, [("add_used", M._u32(dependants), M._u32(used))])

    def release(self, handles):
        for g, hs in zip(self.gs, self._local(handles)):
            if hs:
                g.release(hs)

    def run_batch(self, steps):
        ids, outs, _ = self.fgi.part_local_run_batch(self.gs, steps)
        outs = [self._handles_out(sp[1], o) if sp[0] == "begin_compute" else o for sp, o in zip(steps, outs)]
        return ids, outs

    def tick(self, now, want, roots, detached):
        """The collective tick against the model's: want (None: no wave ran), roots per rank, detached handles per rank."""
        before = self._last_ids()
        fired, det, _ = self.fgi.part_local_timers_run_due(self.gs, now)
        for r, g in enumerate(self.gs):
            assert fired[r] == roots[r] + len(detached[r]), f"rank {r} fired {fired[r]}, the model {roots[r]} + {len(detached[r])}"
            assert det[r] == len(detached[r]), f"rank {r}: {det[r]} detached handles fired, the model {len(detached[r])}"
            local = np.array(sorted(self.block + (h - self.n) % self.n_det for h in detached[r]), np.uint32)
            assert np.array_equal(g.part_timers_fired_detached(), local), f"rank {r}: the fired detached handles"
            assert np.array_equal(g.part_timers_fired_detached(), local), f"rank {r}: a second call returns another list"
        if want is None:
            assert self._last_ids() == before, "a tick that fired no slot changed a rank's last wave"
            return
        for r, ids in enumerate(self._wave_ids("a tick's wave")):
            lo, hi = self._range(r)
            assert np.array_equal(ids, want[(want >= lo) & (want < hi)]), f"rank {r}: the fired timers' wave"

    def _last_ids(self):
        out = []
        for g in self.gs:
            try:
                out.append(g.part_last_wave_ids().tolist())
            except self.pkg.FgiError as e:   # the rank's last call was a mutation or a batch: no wave stands
                out.append(("status", e.status))
        return out

    # ---- what Driver.check reads ----
    def dump_states(self):
        v, f = np.zeros(self.n + self.P * self.n_det, np.uint64), np.zeros(self.n + self.P * self.n_det, np.uint32)
        for r, g in enumerate(self.gs):
            gv, gf = g.dump_states()
            lo, hi = self._range(r)
            v[lo:hi], f[lo:hi] = gv[:hi - lo], gf[:hi - lo]
            assert not gv[hi - lo:self.block].any(), f"rank {r}: a node past the rank's slots"
            d = self.n + r * self.n_det
            v[d:d + self.n_det], f[d:d + self.n_det] = gv[self.block:], gf[self.block:]
        return v, f

    def timers_list(self):
        hs, vs, ds = [], [], []
        for r, g in enumerate(self.gs):
            h, v, d = g.timers_list()
            assert np.all(np.diff(h.astype(np.int64)) > 0), f"rank {r}: fgi_timers_list does not ascend"
            assert np.all((h < self._range(r)[1] - self._range(r)[0]) | (h >= self.block)), f"rank {r}: an entry past its slots"
            hs.append(to_model(self.n, self.block, self.n_det, r, h))
            vs.append(v)
            ds.append(d)
        h, v, d = np.concatenate(hs), np.concatenate(vs), np.concatenate(ds)
        o = np.argsort(h, kind="stable")
        return h[o], v[o], d[o]

    def timers_stats(self):
        per = [g.timers_stats() for g in self.gs]
        assert len({s["runs"] for s in per}) == 1, f"runs differ between the ranks: {[s['runs'] for s in per]}"
        out = {k: sum(s[k] for s in per) for k in ("stored", "armed", "fired", "dropped", "moved")}
        out["runs"] = per[0]["runs"]
        return out

    def timers_next_due(self):
        per = [g.timers_next_due() for g in self.gs]
        return min(d for d, _ in per), sum(s for _, s in per)


def _maker(pkg, P, labels=0, options=None):
    def make(arrays, n_det, **kw):
        n = len(arrays[0])
        gs, block = _build_with(pkg, P, n, *arrays, options=options or {}, labels=labels, n_detached=n_det)
        return PM.PartDriver(arrays, n_det, P, engine=Group(pkg, gs, block, n, n_det), fgi=pkg.fgi, **kw)
    return make


# ---- the scenarios through PartDriver --------------------------------------------------------------------------

@pytest.mark.parametrize("labels", [0, 1])
@pytest.mark.parametrize("scn", ["scn_chain", "scn_cascading", "scn_slot_reuse", "scn_saturation", "scn_open_populated"])
def test_single_device_scenarios_on_two_ranks(pkg, gpu_available, scn, labels):
    drv = getattr(M, scn)(_maker(pkg, 2, labels))
    drv.g.close()


@pytest.mark.parametrize("labels", [0, 1])
def test_edges(pkg, gpu_available, labels):
    """200 slots over three ranks (block 67, the last rank owns 66), 8 detached handles each: a tick only the last
    rank has entries for, a tick of 66 entries of rank 0 alone (local handles 0, 63, 64 and 66 among them), a tick
    with the first slots of ranks 1 and 2, slot 199 and two displaced nodes under their owners' detached handles."""
    drv = PM.scn_part_edges(_maker(pkg, PM.EDGE_P, labels))
    assert drv.block == 67 and drv.ticks[0][0] == [0, 0, 10] and drv.ticks[1][0] == [66, 0, 0]
    assert [len(d) for d in drv.ticks[2][1]] == [1, 0, 1]
    drv.g.close()


@pytest.mark.parametrize("labels", [0, 1])
@pytest.mark.parametrize("P", [2, 3, 8])
def test_mixed_states(pkg, gpu_available, P, labels):
    drv = M.scn_mixed(_maker(pkg, P, labels))
    assert drv.c["fired"] >= 50 and drv.seen["overwrites"] >= 1 and drv.seen["stale"] >= 1
    drv.g.close()


@pytest.mark.parametrize("P", [2, 3])
def test_batch(pkg, gpu_available, P):
    drv = M.scn_batch(_maker(pkg, P))
    assert drv.seen["det_moved"] >= 8 and drv.seen["det_fired"] >= 1
    drv.g.close()


# ---- gates ---------------------------------------------------------------------------------------------------

STAT_FIELDS = ("host_syncs", "levels", "v_inv", "e_trav", "e_match", "n_flagged", "roots", "f_total")


@pytest.mark.parametrize("labels", [0, 1])
def test_twin_groups(pkg, gpu_available, labels):
    """The three _mixed() waves on two groups, timers open on one: the same ids, flagged sets and statistics,
    host_syncs included; the group that never opened timers reports zero fgi_timer_stats."""
    arrays, waves, _ = _mixed()
    a, _ = _build_with(pkg, 3, MIXED_N, *arrays, options={}, labels=labels)
    b, _ = _build_with(pkg, 3, MIXED_N, *arrays, options={}, labels=labels)
    for g in a:
        g.part_timers_open(default_delay=4)
    for roots, imm, *_ in waves:
        sa, sb = pkg.fgi.part_local_invalidate(a, roots, imm), pkg.fgi.part_local_invalidate(b, roots, imm)
        for r, (ga, gb) in enumerate(zip(a, b)):
            assert np.array_equal(ga.part_last_wave_ids(), gb.part_last_wave_ids()), r
            fa, fb = ga.part_last_flagged(), gb.part_last_flagged()
            assert all(np.array_equal(x, y) for x, y in zip(fa, fb)), r
            for k in STAT_FIELDS:
                assert getattr(sa[r], k) == getattr(sb[r], k), (r, k)
    assert sum(g.timers_stats()["stored"] for g in a) > 20
    for g in b:
        assert g.timers_stats() == dict(stored=0, armed=0, fired=0, dropped=0, moved=0, runs=0, last_kernel_ms=0.0)
    for g in a + b:
        g.close()


@pytest.mark.parametrize("coll", [0, 1])
@pytest.mark.parametrize("scn", ["scn_chain", "scn_cascading"])
def test_world_one(pkg, gpu_available, scn, coll):
    """One rank, with and without its collectives, against a single-device engine with fgi_timers_*."""
    part = getattr(M, scn)(_maker(pkg, 1, options={pkg.fgi.OPT_PART_COLLECTIVES: coll}))

    def single(arrays, n_det, **kw):
        return M.Driver(arrays, n_det, engine=_engine(pkg, len(arrays[0]), *arrays, n_detached=n_det), fgi=pkg.fgi, **kw)
    one = getattr(M, scn)(single)
    assert part.c == one.c
    assert all(np.array_equal(x, y) for x, y in zip(part.g.timers_list(), one.g.timers_list()))
    ps, os_ = part.g.timers_stats(), one.g.timers_stats()
    assert all(ps[k] == os_[k] for k in ps)
    assert np.array_equal(part.g.gs[0].part_last_wave_ids(), one.g.last_wave_ids())
    part.g.close()


def _chain_group(pkg, P=2, n_det=4, labels=0):
    """scn_chain's graph, 0 -> 1 -> 2 -> 3 (delay 5) -> 4, over P ranks."""
    arrays = M.chain_arrays(5, [(0, 1), (1, 2), (2, 3), (3, 4)], delayed=[3])
    gs, block = _build_with(pkg, P, 5, *arrays, options={}, labels=labels, n_detached=n_det)
    return gs, block, arrays


def test_follow_ons_of_a_timer_wave(pkg, gpu_available):
    fgi = pkg.fgi
    gs, block, _ = _chain_group(pkg)
    assert block == 3
    views = [g.part_open_state_view()[0] for g in gs]
    for g in gs:
        g.part_timers_open(default_delay=5)
    for g in gs:   # slot 3 and 4 are rank 1's
        g.part_subscribe([3, 4], [0, 1], [30, 40])
    fgi.part_local_invalidate(gs, [0])
    assert fgi.part_view_is_consistent(views, block, 3)
    fired, det, stats = fgi.part_local_timers_run_due(gs, 5)
    assert fired == [0, 1] and det == [0, 0]
    off, calls, slots = gs[1].part_last_wave_fanout(2)
    assert list(off) == [0, 1, 2] and list(calls) == [30, 40] and list(slots) == [3, 4]
    assert len(gs[0].part_last_wave_fanout(2)[1]) == 0
    assert not fgi.part_view_is_consistent(views, block, 3) and not fgi.part_view_is_consistent(views, block, 4)
    assert list(gs[1].part_last_wave_ids()) == [3, 4] and list(gs[0].part_last_wave_ids()) == []
    _, fl_ids, _ = gs[1].part_last_flagged()
    assert len(fl_ids) == 0
    fired, det, _ = fgi.part_local_timers_run_due(gs, 6)   # nothing fired: the previous wave stands
    assert fired == [0, 0] and list(gs[1].part_last_wave_ids()) == [3, 4]
    assert [g.timers_stats()["runs"] for g in gs] == [1, 1]
    for g in gs:
        g.close()


def _tick_each(pkg, gs, now):
    """fgi_part_timers_run_due on one thread per rank: every rank's status."""
    def one(r, g):
        try:
            g.part_timers_run_due(now)
            return pkg.fgi.OK
        except pkg.FgiError as e:
            return e.status
    return _each_rank(gs, one)


def test_refusals(pkg, gpu_available):
    fgi = pkg.fgi
    arrays = M.chain_arrays(5, [(0, 1), (1, 2), (2, 3), (3, 4)], delayed=[3])
    single = _engine(pkg, 5, *arrays, n_detached=0)
    with pytest.raises(pkg.FgiError) as e:
        single.part_timers_open()
    assert e.value.status == fgi.ENOTSUP
    gs, block, _ = _chain_group(pkg)
    gs[0].part_timers_open(now=10)
    # one rank not open: the same FGI_ESTATE everywhere, nothing removed
    gs[0].part_timers_set_delay([0, 1, 3], [5, 5, 5])
    assert _tick_each(pkg, gs, 11) == [fgi.ESTATE, fgi.ESTATE]
    gs[1].part_timers_open(now=10)
    for g in gs:
        with pytest.raises(pkg.FgiError) as e:
            g.part_timers_open()
        assert e.value.status == fgi.ESTATE
        for call in (lambda: g.timers_set_delay([0], [5]), lambda: g.timers_run_due(11)):
            with pytest.raises(pkg.FgiError) as e:
                call()
            assert e.value.status == fgi.ENOTSUP
    gs[1].part_timers_set_delay([3], [5])
    for bad in ([5], [3, 3], [1, 3, 1]):
        with pytest.raises(pkg.FgiError) as e:
            gs[1].part_timers_set_delay(bad, [9] * len(bad))
        assert e.value.status == fgi.EINVAL
    fgi.part_local_invalidate(gs, [0])
    listed = [[a.tolist() for a in g.timers_list()] for g in gs]
    assert listed[0] == [[], [], []] and listed[1][0] == [0] and listed[1][2] == [15]   # the refused delay 9 was not stored
    # the clock: below it is FGI_EINVAL everywhere and changes nothing
    assert _tick_each(pkg, gs, 9) == [fgi.EINVAL, fgi.EINVAL]
    gs[0].timers_set_now(12)   # the ranks' clocks may differ; a `now` below any of them is refused by all
    assert _tick_each(pkg, gs, 11) == [fgi.EINVAL, fgi.EINVAL]
    assert [[a.tolist() for a in g.timers_list()] for g in gs] == listed
    assert [g.timers_stats()["fired"] for g in gs] == [0, 0]
    # ranks that disagree about `now`
    got = _each_rank(gs, lambda r, g: _status(pkg, lambda: g.part_timers_run_due(20 + r)))
    assert got == [fgi.EINVAL, fgi.EINVAL] and [[a.tolist() for a in g.timers_list()] for g in gs] == listed
    # one rank closed while the other holds an entry that is due: the same FGI_ESTATE on both, and the open rank
    # removes nothing (the agreement comes before the due pass)
    gs[0].timers_close()
    before = gs[1].timers_stats()
    assert before["stored"] == 1 and listed[1][2] == [15]
    assert _tick_each(pkg, gs, 15) == [fgi.ESTATE, fgi.ESTATE]
    assert [a.tolist() for a in gs[1].timers_list()] == listed[1]
    after = gs[1].timers_stats()
    assert all(after[k] == before[k] for k in ("stored", "armed", "fired", "dropped", "moved", "runs")), (before, after)
    assert gs[1].timers_next_due() == (15, 1)
    assert gs[0].timers_stats()["armed"] == 0   # closed: zeros
    gs[0].part_timers_open(now=12)
    # a short cap: the wave has run
    def short(r, g):
        ids, n, fired = np.zeros(1, np.uint32), C.c_uint64(), C.c_uint64()
        st = g.lib.fgi_part_timers_run_due(g.h, 15, ids.ctypes.data_as(C.POINTER(C.c_uint32)), 1, C.byref(n), C.byref(fired),
                                           None, None)
        return st, n.value, fired.value
    assert _each_rank(gs, short) == [(fgi.OK, 0, 0), (fgi.ECAPACITY, 2, 1)]
    assert list(gs[1].part_last_wave_ids()) == [3, 4]
    for g in gs:
        g.close()


def _status(pkg, call):
    try:
        call()
        return pkg.fgi.OK
    except pkg.FgiError as e:
        return e.status


def test_restore_release_and_close(pkg, gpu_available):
    """fgi_restore on a rank drops its entries (counted) and keeps its clock and delays; fgi_release drops the
    entry of a detached handle; after fgi_timers_close the rank's waves arm nothing and it may open again."""
    fgi = pkg.fgi
    gs, block, arrays = _chain_group(pkg)
    for g in gs:
        g.part_timers_open(now=3)
        g.part_timers_set_delay([3], [5])
        g.snapshot()
    fgi.part_local_invalidate(gs, [0])
    assert [g.timers_stats()["stored"] for g in gs] == [0, 1]
    for g in gs:
        g.restore()
    st = gs[1].timers_stats()
    assert st["stored"] == 0 and st["dropped"] == 1 and st["armed"] == 1 and len(gs[1].timers_list()[0]) == 0
    fgi.part_local_invalidate(gs, [0])   # the clock and the delay stayed
    assert [a.tolist() for a in gs[1].timers_list()[::2]] == [[0], [8]]
    # the node of slot 3 displaced with its entry, then released
    v = arrays[0]
    _, outs, _ = fgi.part_local_run_batch(gs, [("begin_compute", np.array([3], np.uint32), v[[3]] + np.uint64(7))])
    d = int(outs[0][0])
    assert d >= block and gs[1].timers_list()[0].tolist() == [d] and gs[1].timers_stats()["moved"] == 1
    gs[1].release([d])
    st = gs[1].timers_stats()
    assert st["stored"] == 0 and st["dropped"] == 2 and st["armed"] == 2
    gs[1].timers_close()
    assert gs[1].timers_stats()["armed"] == 0
    gs[1].part_timers_open()
    for g in gs:
        g.close()


def test_direct_entry_points_arm(pkg, gpu_available):
    """fgi_part_invalidate_host, fgi_part_begin_compute and fgi_part_set_output called rank by rank (not through a
    batch) arm behind their cascades as the batch forms do."""
    fgi = pkg.fgi
    gs, block, arrays = _chain_group(pkg)
    for g in gs:
        g.part_timers_open(default_delay=5)
    _each_rank(gs, lambda r, g: g.part_invalidate_host([0]))
    assert [g.timers_list()[0].tolist() for g in gs] == [[], [0]]
    # slot 3's node moves to a detached handle with its entry; slot 3 is computed again and set
    v = arrays[0]
    outs = _each_rank(gs, lambda r, g: g.part_begin_compute([3], v[[3]] + np.uint64(9), [1])[0])
    d = int(outs[1][0])
    assert d >= block and outs[0][0] == NONE and gs[1].timers_list()[0].tolist() == [d]
    _each_rank(gs, lambda r, g: g.part_set_output([3]))
    assert gs[1].timers_stats()["moved"] == 1 and gs[1].timers_stats()["armed"] == 1
    fired = _each_rank(gs, lambda r, g: g.part_timers_run_due(5)[1:])
    assert fired == [(0, 0), (1, 1)] and gs[1].part_timers_fired_detached().tolist() == [d]
    for g in gs:
        g.close()


# ---- two real processes --------------------------------------------------------------------------------------

def test_edges_across_processes(gpu_available, tmp_path):
    """The edges graph over two processes (host all-gathers over gloo) through Graph.part_timers_run_due: each
    rank's ids, entries and counts against the model run here."""
    out = tmp_path / "p2"
    out.mkdir()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "part_timers_worker.py"), "--out", str(out)]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    ranks = [dict(np.load(out / f"rank{q}.npz")) for q in range(2)]
    P, n, n_det = 2, PM.EDGE_N, PM.EDGE_DET
    arrays, others, delays = PM.edge_plan(n, P)
    drv = PM.PartDriver(arrays, n_det, P)
    block = drv.block

    def compare(k, want, fired=None):
        mh, mv, md = drv.listed()
        ov, of = drv.states()
        for q, res in enumerate(ranks):
            lo, hi = q * block, min(n, (q + 1) * block)
            if want is not None:
                assert np.array_equal(res[f"s{k}_ids"], want[(want >= lo) & (want < hi)]), f"step {k}, rank {q}: ids"
            h = to_model(n, block, n_det, q, res[f"s{k}_h"])
            mine = np.array([drv.owner(x) == q for x in mh], bool)
            assert np.array_equal(h, mh[mine]) and np.array_equal(res[f"s{k}_v"], mv[mine]), f"step {k}, rank {q}: entries"
            assert np.array_equal(res[f"s{k}_d"], md[mine]), f"step {k}, rank {q}: due times"
            gv, gf = res[f"s{k}_sv"], res[f"s{k}_sf"]
            assert np.array_equal(gv[:hi - lo], ov[lo:hi]) and np.array_equal(gf[:hi - lo], of[lo:hi]), f"step {k}, rank {q}: states"
            d = n + q * n_det
            assert np.array_equal(gv[block:], ov[d:d + n_det]) and np.array_equal(gf[block:], of[d:d + n_det])
            if fired is not None:
                roots, det = drv.ticks[-1]
                assert res[f"s{k}_fired"].tolist() == [roots[q] + len(det[q]), len(det[q])], f"step {k}, rank {q}: counts"
                assert to_model(n, block, n_det, q, res[f"s{k}_fdet"]).tolist() == sorted(det[q])
        assert sum(int(res[f"s{k}_runs"][0]) for res in ranks) == 2 * drv.c["runs"]

    drv.open()
    drv.set_delay(others, delays[others])
    compare(0, drv.invalidate([PM.EDGE_HUB]))
    compare(1, drv.tick(1)[0], True)
    # the detached handles the owners handed out
    handles = np.array([NONE if ranks[s // block]["moved"][i] == NONE
                        else to_model(n, block, n_det, s // block, [ranks[s // block]["moved"][i]])[0]
                        for i, s in enumerate(PM.EDGE_MOVED)], np.uint32)
    drv._fed = [handles]
    v = drv.states()[0]
    drv.begin_compute(PM.EDGE_MOVED, v[PM.EDGE_MOVED] + np.uint64(10))
    assert drv.c["moved"] == 2
    compare(2, None)
    for k, now in ((3, 2), (4, 3), (5, 4), (6, 50)):
        want, fired = drv.tick(now)
        compare(k, want if drv.ticks[-1][0] != [0, 0] else None, True)
    assert not drv.entries and drv.seen["det_fired"] == 2
