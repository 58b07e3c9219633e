"""The auto-invalidation timers per rank of a partition (fgi_part_timers_auto_*, fgi_part_set_output_ex, C-ABI 0.14)
against the model of test_part_auto_timers_model.py.

The ranks are in-process groups on one GPU (`_build_with`). `AutoGroup` is test_gpu_part_timers.py's `Group` with
the calls `AutoDriver` makes besides: every rank is handed every list whole and keeps its share; set_output goes
through fgi_part_local_run_batch as a one-step batch with the step's transient flags. After every step the engine
must equal the model, per rank, in the invalidated ids, fgi_dump_states, fgi_part_timers_list_ex (kinds
included), the fired and detached counts, fgi_timers_next_due, the summed fgi_timer_stats and the summed auto
statistics. Expected values never come from the engine; the one thing the model takes from it is which detached
handle a displaced node was given. The gates at the end check what the model does not cover."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_flagged import _engine
from test_gpu_part_host import _free_port
from test_gpu_part_state_view import _build_with, _each_rank
from test_gpu_part_timers import Group, to_model
import test_auto_timers_model as A
import test_part_auto_timers_model as PA
import test_timers_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ZERO = dict(armed_auto=0, merged=0, fired_auto=0)


class AutoGroup(Group):
    def timers_auto_open(self, default_auto=0, default_transient=0):
        for g in self.gs:
            g.part_timers_auto_open(default_auto, default_transient)

    def timers_set_auto_delay(self, handles, auto=None, transient=None):
        for g in self.gs:
            g.part_timers_set_auto_delay(handles, auto, transient)

    def timers_start_auto(self, handles, transient=None):
        for g in self.gs:
            g.part_timers_start_auto(handles, transient)

    def set_output(self, handles, transient=None):
        step = ("set_output", M._u32(handles)) + (() if transient is None else (np.asarray(transient, np.uint8),))
        _, outs, _ = self.fgi.part_local_run_batch(self.gs, [step])
        return outs[0], None

    def timers_list_ex(self):
        hs, vs, ds, ks = [], [], [], []
        for r, g in enumerate(self.gs):
            h, v, d, k = g.part_timers_list_ex()
            assert np.all(np.diff(h.astype(np.int64)) > 0), f"rank {r}: fgi_part_timers_list_ex does not ascend"
            assert np.all((h < self._range(r)[1] - self._range(r)[0]) | (h >= self.block)), f"rank {r}: an entry past its slots"
            h3, v3, d3 = g.timers_list()
            assert np.array_equal(h, h3) and np.array_equal(v, v3) and np.array_equal(d, d3), f"rank {r}: the two lists differ"
            hs.append(to_model(self.n, self.block, self.n_det, r, h))
            vs.append(v)
            ds.append(d)
            ks.append(k)
        h, v, d, k = np.concatenate(hs), np.concatenate(vs), np.concatenate(ds), np.concatenate(ks)
        o = np.argsort(h, kind="stable")
        return h[o], v[o], d[o], k[o]

    def timers_auto_stats(self):
        per = [g.part_timers_auto_stats() for g in self.gs]
        return {k: sum(s[k] for s in per) for k in ZERO}


def _group(pkg, P, arrays, n_det, labels=0):
    arrays = PA.pad_arrays(arrays, P)
    n = len(arrays[0])
    gs, block = _build_with(pkg, P, n, *arrays, options={}, labels=labels, n_detached=n_det)
    return arrays, AutoGroup(pkg, gs, block, n, n_det)


def _maker(pkg, P, labels=0):
    def make(arrays, n_det, **kw):
        arrays, group = _group(pkg, P, arrays, n_det, labels)
        return PA.PartAutoDriver(arrays, n_det, P, engine=group, fgi=pkg.fgi, **kw)
    return make


# ---- the scenarios through PartAutoDriver ------------------------------------------------------------------------

@pytest.mark.parametrize("labels", [0, 1])
@pytest.mark.parametrize("P", PA.RANKS)
@pytest.mark.parametrize("scn", PA.INHERITED)
def test_single_device_scenarios_over_ranks(pkg, gpu_available, scn, P, labels):
    drv = getattr(A, scn)(_maker(pkg, P, labels))
    assert drv.n % P != 0 and drv.auto
    drv.g.close()


@pytest.mark.parametrize("labels", [0, 1])
@pytest.mark.parametrize("P", PA.RANKS)
def test_displacement(pkg, gpu_available, P, labels):
    """An auto entry moved to a detached handle and fired there, on two ranks: reported, not cascaded."""
    drv = PA.scn_part_displacement(_maker(pkg, P, labels))
    assert drv.seen["det_fired_auto"] == 2 and drv.ca["fired_auto"] == 2
    drv.g.close()


@pytest.mark.parametrize("labels", [0, 1])
@pytest.mark.parametrize("P", PA.RANKS)
def test_batch(pkg, gpu_available, P, labels):
    """The partition's step-by-step batch rule: a stale entry behind an invalidated node, an entry moved with its
    displaced node and merged with the delay arm, an overwrite by the second set_output of one batch."""
    drv = PA.scn_part_batch(_maker(pkg, P, labels))
    assert drv.seen["batch_stale"] == 2 and drv.seen["batch_moved_auto"] == 2 and drv.seen["batch_overwrites"] == 1
    drv.g.close()


@pytest.mark.parametrize("labels", [0, 1])
@pytest.mark.parametrize("P", PA.RANKS)
def test_divergence_shape(pkg, gpu_available, P, labels):
    """One set_output / start_auto list, whole on every rank, in which owned and unowned slots alternate item by
    item and unset, InvalidateOnSetOutput and transient items are mixed in: a lane that left before tm_store would
    show as wrong counters or a lost entry."""
    drv = PA.scn_divergence(_maker(pkg, P, labels), P)
    assert drv.seen["ioso"] == 50 and drv.ca["merged"] >= 50
    drv.g.close()


def test_past_one_grid(pkg, gpu_available):
    """More than 1,024 x 256 owned candidates on a rank, through start_auto and through set_output (the sizes:
    test_part_auto_timers_model.py's test_past_one_grid_model)."""
    drv = PA.scn_part_past_one_grid(_maker(pkg, PA.GRID_P))
    assert drv.ca == dict(armed_auto=PA.GRID_N, merged=0, fired_auto=PA.GRID_N)
    drv.g.close()


@pytest.mark.parametrize("labels", [0, 1])
@pytest.mark.parametrize("P", PA.RANKS)
def test_parity_with_one_device(pkg, gpu_available, P, labels):
    """Single calls only: the union of the ranks' list_ex, as global slots, is a single-device engine's
    fgi_timers_list_ex, and the summed counters are its counters."""
    def single(arrays, n_det, **kw):
        arrays = PA.pad_arrays(arrays, P)
        return A.AutoDriver(arrays, n_det, engine=_engine(pkg, len(arrays[0]), *arrays, n_detached=n_det), fgi=pkg.fgi, **kw)

    def same(part, one, stored):
        assert part.c == one.c and part.ca == one.ca and not part.det
        pl, ol = part.g.timers_list_ex(), one.g.timers_list_ex()   # (no detached handle: model handles are global slots)
        assert stored == (len(ol[0]) > 0)
        assert all(np.array_equal(x, y) for x, y in zip(pl, ol))
        ps, os_ = part.g.timers_stats(), one.g.timers_stats()
        assert all(ps[k] == os_[k] for k in ps)
        assert part.g.timers_auto_stats() == one.g.timers_auto_stats()
        part.g.close()

    same(_until_first_tick(PA.scn_parity, _maker(pkg, P, labels)), _until_first_tick(PA.scn_parity, single), True)
    same(PA.scn_parity(_maker(pkg, P, labels)), PA.scn_parity(single), False)


class _Stop(Exception):
    pass


def _until_first_tick(scn, make):
    """The scenario up to its first tick (entries stored on every rank)."""
    made = []

    def wrapped(arrays, n_det, **kw):
        drv = make(arrays, n_det, **kw)

        def stop(now):
            raise _Stop()
        drv.tick = stop
        made.append(drv)
        return drv
    with pytest.raises(_Stop):
        scn(wrapped)
    return made[0]


# ---- fgi_part_set_output_ex itself ----------------------------------------------------------------------------

def _begun_groups(pkg, P, labels, auto=True, count=2):
    """`count` identical groups over 100 slots (block 34 at P = 3: the last rank owns 32): hub 0 Consistent, slots
    1..89 freshly begun, every seventh of them flagged InvalidateOnSetOutput by a cascade from the hub."""
    n = 100
    arrays = PA.pad_arrays(A.slot_arrays(n, consistent=[0, 95], edges=[(0, 95)]), P)   # (a bulk edge: partition codes)
    s = np.arange(1, 90, dtype=np.uint32)
    ioso = s[s % 7 == 0]
    groups = []
    for _ in range(count):
        gs, block = _build_with(pkg, P, len(arrays[0]), *arrays, options={}, labels=labels, n_detached=4)
        for g in gs:
            g.part_timers_open(default_delay=0, now=5)
            if auto:
                g.part_timers_auto_open(9, 3)
                g.part_timers_set_auto_delay(s[::5], np.full(len(s[::5]), 4, np.uint64))
        pkg.fgi.part_local_run_batch(gs, [("begin_compute", s, s.astype(np.uint64) + np.uint64(900)),
                                          ("add_used", ioso, np.zeros(len(ioso), np.uint32))])
        pkg.fgi.part_local_invalidate(gs, [0])
        groups.append(gs)
    order = PA.divergence_order(len(arrays[0]), P)
    return groups, order, (order % 3 == 0).astype(np.uint8), block


def _rank_lists(gs):
    return [[a.tolist() for a in g.part_timers_list_ex()] for g in gs]


@pytest.mark.parametrize("labels", [0, 1])
@pytest.mark.parametrize("P", PA.RANKS)
def test_set_output_ex_equals_the_batch_step(pkg, gpu_available, P, labels):
    """fgi_part_set_output_ex on one host thread per rank against the same step through fgi_part_local_run_batch."""
    (a, b), order, tr, block = _begun_groups(pkg, P, labels)
    res = _each_rank(a, lambda r, g: g.part_set_output(order, transient=tr))
    ids_b, outs_b, _ = pkg.fgi.part_local_run_batch(b, [("set_output", order, tr)])
    for r in range(P):
        assert np.array_equal(res[r][0], outs_b[0]), f"rank {r}: out_set"
    assert np.array_equal(np.sort(np.concatenate([x[1] for x in res])), np.sort(ids_b))
    s = order[(order >= 1) & (order < 90)]
    assert sorted(s[s % 7 == 0].tolist()) == sorted(ids_b.tolist()), "the InvalidateOnSetOutput items' cascade"
    assert _rank_lists(a) == _rank_lists(b)
    want = {int(h): 5 + (3 if h % 3 == 0 else 4 if (h - 1) % 5 == 0 else 9) for h in s if h % 7 != 0}
    got = {}
    for r, g in enumerate(a):
        h, v, d, k = g.part_timers_list_ex()
        assert np.all(k == 1) and np.all(h < block)
        got.update({r * block + int(x): int(y) for x, y in zip(h, d)})
        assert np.array_equal(v, (r * block + h).astype(np.uint64) + np.uint64(900))
    assert got == want
    assert [g.part_timers_auto_stats() for g in a] == [g.part_timers_auto_stats() for g in b]
    assert sum(g.part_timers_auto_stats()["armed_auto"] for g in a) == len(want)
    for g in a + b:
        g.close()


# ---- gates ---------------------------------------------------------------------------------------------------

def _status(pkg, call):
    try:
        call()
        return pkg.fgi.OK
    except pkg.FgiError as e:
        return e.status


def test_status_codes(pkg, gpu_available):
    fgi = pkg.fgi
    arrays = A.slot_arrays(8, consistent=[0, 5])
    single = _engine(pkg, 8, *arrays, n_detached=0)
    single.timers_open()
    for call in (lambda: single.part_timers_auto_open(), lambda: single.part_timers_set_auto_delay([1], [2]),
                 lambda: single.part_set_output([1], transient=[0]), lambda: single.part_timers_start_auto([0]),
                 lambda: single.part_timers_auto_stats(), lambda: single.part_timers_list_ex()):
        assert _status(pkg, call) == fgi.ENOTSUP
    _, group = _group(pkg, 2, arrays, 2)
    gs = group.gs
    g = gs[0]
    assert _status(pkg, lambda: g.part_timers_auto_open()) == fgi.ESTATE           # before fgi_part_timers_open
    assert g.part_timers_auto_stats() == ZERO
    for x in gs:
        x.part_timers_open(default_delay=3)
    assert _status(pkg, lambda: g.part_timers_set_auto_delay([1], [2])) == fgi.ESTATE   # before auto_open
    assert _status(pkg, lambda: g.part_timers_start_auto([0])) == fgi.ESTATE
    assert g.part_timers_auto_stats() == ZERO and [len(a) for a in g.part_timers_list_ex()] == [0] * 4
    for x in gs:
        x.part_timers_auto_open(7, 0)
    assert _status(pkg, lambda: g.part_timers_auto_open()) == fgi.ESTATE           # already on
    for bad in ([group.n], [1, 1], [1, 6, 1]):
        assert _status(pkg, lambda: g.part_timers_set_auto_delay(bad, [9] * len(bad))) == fgi.EINVAL
        assert _status(pkg, lambda: g.part_timers_start_auto(bad)) == fgi.EINVAL
    # the 0.13 names on a rank with auto open
    for call in (lambda: g.timers_auto_open(), lambda: g.timers_set_auto_delay([1], [2]), lambda: g.set_output([1], transient=[0]),
                 lambda: g.timers_start_auto([0]), lambda: g.timers_auto_stats(), lambda: g.timers_list_ex()):
        assert _status(pkg, call) == fgi.ENOTSUP
    # slots of the other rank are skipped, and nothing of a refused list was stored
    for x in gs:
        x.part_timers_start_auto([0, 5])
    assert [x.part_timers_list_ex()[0].tolist() for x in gs] == [[0], [5 - group.block]]
    assert [x.part_timers_list_ex()[2].tolist() for x in gs] == [[7], [7]]
    assert [x.part_timers_auto_stats()["armed_auto"] for x in gs] == [1, 1]
    group.close()


def test_restore_and_close(pkg, gpu_available):
    """fgi_restore keeps the auto delays and counters and drops the entries; fgi_timers_close turns auto off."""
    fgi = pkg.fgi
    _, group = _group(pkg, 2, A.slot_arrays(8, consistent=[0, 5]), 2)
    gs = group.gs
    for g in gs:
        g.part_timers_open(now=1)
        g.part_timers_auto_open(0, 0)
        g.part_timers_set_auto_delay([0, 5], [4, 6])
        g.snapshot()
        g.part_timers_start_auto([0, 5])
    assert [g.part_timers_list_ex()[2].tolist() for g in gs] == [[5], [7]]
    for g in gs:
        g.restore()
    for g in gs:
        assert len(g.part_timers_list_ex()[0]) == 0
        assert g.part_timers_auto_stats() == dict(armed_auto=1, merged=0, fired_auto=0)
        st = g.timers_stats()
        assert st["armed"] == 1 and st["dropped"] == 1 and st["stored"] == 0
        g.part_timers_start_auto([0, 5])               # the delays stayed
    assert [g.part_timers_list_ex()[2].tolist() for g in gs] == [[5], [7]]
    assert [g.part_timers_list_ex()[3].tolist() for g in gs] == [[1], [1]]
    gs[0].timers_close()
    assert gs[0].part_timers_auto_stats() == ZERO
    gs[0].part_timers_open()
    assert _status(pkg, lambda: gs[0].part_timers_start_auto([0])) == fgi.ESTATE
    assert gs[0].part_timers_auto_stats() == ZERO
    group.close()


STAT_FIELDS = ("host_syncs", "levels", "v_inv", "e_trav", "e_match", "n_flagged", "roots", "f_total")


@pytest.mark.parametrize("labels", [0, 1])
def test_inert_without_auto(pkg, gpu_available, labels):
    """Part timers open, auto never: the same step with and without transient flags leaves identical lists and
    counters, and host_syncs equal a group's with auto open (the auto arm adds no wait)."""
    P = 3
    (plain, flagged, opened), order, tr, _ = _begun_groups(pkg, P, labels, auto=False, count=3)
    for g in opened:
        g.part_timers_auto_open(9, 3)
    for g in plain + flagged + opened:
        g.part_timers_set_delay([0], [5])
    stats = []
    for gs, t in ((plain, None), (flagged, tr), (opened, tr)):
        ws = [pkg.WaveStats() for _ in gs]
        stats.append(ws)
        _each_rank(gs, lambda r, g: g.part_set_output(order, stats=ws[r], transient=t))
    for r in range(P):
        for k in STAT_FIELDS:
            assert getattr(stats[0][r], k) == getattr(stats[1][r], k) == getattr(stats[2][r], k), (r, k)
    b1 = pkg.fgi.part_local_run_batch(plain, [("begin_compute", [1, 40, 80], [7001, 7040, 7080]), ("set_output", [1, 40, 80])])
    b2 = pkg.fgi.part_local_run_batch(flagged, [("begin_compute", [1, 40, 80], [7001, 7040, 7080]), ("set_output", [1, 40, 80], [1, 0, 1])])
    assert np.array_equal(b1[0], b2[0]) and all(np.array_equal(x, y) for x, y in zip(b1[1], b2[1]))
    assert [s.host_syncs for s in b1[2]] == [s.host_syncs for s in b2[2]]
    for ga, gb in zip(plain, flagged):
        assert ga.part_timers_auto_stats() == gb.part_timers_auto_stats() == ZERO
        sa, sb = ga.timers_stats(), gb.timers_stats()
        assert all(sa[k] == sb[k] for k in sa if k != "last_kernel_ms")
        la, lb = ga.part_timers_list_ex(), gb.part_timers_list_ex()
        assert all(np.array_equal(x, y) for x, y in zip(la, lb)) and not la[3].any()
        assert np.array_equal(ga.dump_states()[1], gb.dump_states()[1])
    assert sum(g.part_timers_auto_stats()["armed_auto"] for g in opened) > 50
    for g in plain + flagged + opened:
        g.close()


# ---- two real processes --------------------------------------------------------------------------------------

def test_across_processes(gpu_available, tmp_path):
    """Two processes (host all-gathers over gloo), each under its own timeout: fgi_part_set_output_ex with mixed
    transient flags, a tick that fires auto entries on both ranks, one displaced auto entry reported detached; each
    rank's list_ex, states and counters against the model run here."""
    W = PA.ProcPlan
    out = tmp_path / "p2"
    out.mkdir()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.update(OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "part_auto_timers_worker.py"), "--out", str(out)],
                              env=dict(env, RANK=str(q), LOCAL_RANK=str(q)), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for q in range(2)]
    try:
        ends = [p.communicate(timeout=100) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    for p, (_, err) in zip(procs, ends):
        assert p.returncode == 0, err[-3000:]
    ranks = [dict(np.load(out / f"rank{q}.npz")) for q in range(2)]
    P, n, n_det = 2, W.N, W.N_DET
    drv = PA.PartAutoDriver(W.arrays(), n_det, P, **W.DEFAULTS)
    assert PA.padded_n(n, P) == n
    block = drv.block

    def compare(k, want, fired=False):
        mh, mv, md = drv.listed()
        mk = drv.kinds()
        ov, of = drv.states()
        for q, res in enumerate(ranks):
            lo, hi = q * block, min(n, (q + 1) * block)
            if want is not None:
                assert np.array_equal(res[f"s{k}_ids"], want[(want >= lo) & (want < hi)]), f"step {k}, rank {q}: ids"
            h = to_model(n, block, n_det, q, res[f"s{k}_h"])
            mine = np.array([drv.owner(x) == q for x in mh], bool)
            assert np.array_equal(h, mh[mine]) and np.array_equal(res[f"s{k}_v"], mv[mine]), f"step {k}, rank {q}: entries"
            assert np.array_equal(res[f"s{k}_d"], md[mine]) and np.array_equal(res[f"s{k}_k"], mk[mine]), f"step {k}, rank {q}: due, kinds"
            gv, gf = res[f"s{k}_sv"], res[f"s{k}_sf"]
            assert np.array_equal(gv[:hi - lo], ov[lo:hi]) and np.array_equal(gf[:hi - lo], of[lo:hi]), f"step {k}, rank {q}: states"
            d = n + q * n_det
            assert np.array_equal(gv[block:], ov[d:d + n_det]) and np.array_equal(gf[block:], of[d:d + n_det])
            if fired:
                roots, det = drv.ticks[-1]
                assert res[f"s{k}_fired"].tolist() == [roots[q] + len(det[q]), len(det[q])], f"step {k}, rank {q}: counts"
                assert to_model(n, block, n_det, q, res[f"s{k}_fdet"]).tolist() == sorted(det[q])
        for key, table in (("auto", drv.ca), ("stats", drv.c)):
            names = list(ZERO) if key == "auto" else ["armed", "fired", "dropped", "moved"]
            total = sum(ranks[q][f"s{k}_{key}"].astype(np.int64) for q in range(P))
            assert total.tolist() == [table[x] for x in names], (k, key, total, table)

    drv.open()
    drv.auto_open()
    drv.set_auto_delay(W.SLOTS, W.AUTO_DELAYS, W.TRANS_DELAYS)
    drv.set_delay(W.DELAYED, [W.DELAY] * len(W.DELAYED))
    drv.begin_compute(W.SLOTS, W.VERSIONS, W.HAS_DELAY)
    drv.set_output(W.SLOTS, transient=W.TRANSIENT)
    compare(0, None)
    assert len(drv.entries) == len(W.SLOTS) and {drv.entries[int(h)][1] for h in W.SLOTS} == {2, 6}
    want, fired = drv.tick(W.TICKS[0])
    assert all(x > 0 for x in drv.ticks[-1][0]), "the tick fires auto entries on both ranks"
    compare(1, want, True)
    drv.set_now(W.MOVE_AT)
    handles = np.array([0xFFFFFFFF if ranks[int(s) // block]["moved"][i] == 0xFFFFFFFF
                        else to_model(n, block, n_det, int(s) // block, [ranks[int(s) // block]["moved"][i]])[0]
                        for i, s in enumerate(W.MOVED)], np.uint32)
    drv._fed = [handles]
    drv.begin_compute(W.MOVED, W.MOVED_VERSIONS)
    assert drv.c["moved"] == 1 and drv.ca["merged"] == 1
    compare(2, None)
    want, fired = drv.tick(W.TICKS[1])
    assert drv.seen["det_fired_auto"] == 1 and fired == 1 and len(want) == 0
    compare(3, None, True)
    want, fired = drv.tick(W.TICKS[2])
    compare(4, want, True)
    assert drv.ca["fired_auto"] >= 4
