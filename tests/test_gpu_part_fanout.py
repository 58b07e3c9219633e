"""The replica fan-out per rank of a partition (fgi_part_subscribe, fgi_part_last_wave_fanout,
fgi_part_fanout_ids, fgi_part_fanout_detached, fgi_part_unsubscribe_peer; C-ABI 0.10) against a numpy join.

Expected lists are never taken from the engine: they are the test's own subscription arrays joined in numpy
(`np_join` of test_gpu_fanout.py) with the CPU oracle's invalidated set, restricted to the rank's slot range
[r * block, min(n, (r + 1) * block)). The ranks are in-process groups on one GPU; the fan-out calls are made
rank by rank from the test thread (they join no collective).

(labels, FGI_OPT_FANOUT_PATH): with labels = 1 the ranks' engines run on partition codes, so the bitmap form
goes through k_fo_probe (or the host-order bitmap where an accessor made it) and the list form through
part_out_ids; without codes the bitmap form reads the wave's bitmap in place."""
import ctypes as C

import numpy as np
import pytest

import fgo as O
from harness import CONSISTENT, F_HD
from test_gpu_fanout import RSEED, _rmat16, assert_fanout, np_join
from test_gpu_flagged import N, _mixed
from test_gpu_part_host_roots import _chain, _range
from test_gpu_part_state_view import _build_with, _each_rank
from test_gpu_state_view import _mixed_states
from test_part_fanout_abi import MIXED_PEERS, mixed_subscriptions

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
_U32P, _U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
CODES = [(0, 1), (0, 2), (1, 1), (1, 2)]
# and the automatic rule, and the measurement form (the bitmap renumbered whole inside the call; 2 without codes)
CODES_AUTO = CODES + [(1, 0), (1, 3), (0, 3)]


def rank_join(inv, sh, sp, sc, n_peers, lo, hi):
    """np_join over the entries of slots [lo, hi)."""
    m = (sh >= lo) & (sh < hi)
    return np_join(inv, sh[m], sp[m], sc[m], n_peers)


def _set_path(pkg, gs, path):
    for g in gs:
        g.set_option(pkg.fgi.OPT_FANOUT_PATH, path)


def _subscribe_all(pkg, gs, block, sh, sp, sc):
    """Every rank is handed the whole list: SUB_NOT_OWNED everywhere but on the owner; returns the owners' results."""
    res = np.full(len(sh), NONE, np.uint32)
    for r, g in enumerate(gs):
        got = g.part_subscribe(sh, sp, sc)
        own = sh // block == r
        assert np.all(got[~own] == pkg.fgi.SUB_NOT_OWNED), f"rank {r}: an entry of another rank's slot"
        assert np.all(got[own] != pkg.fgi.SUB_NOT_OWNED), f"rank {r}: an owned slot refused"
        res[own] = got[own]
    return res


def _live(gs):
    return sum(g.sub_stats()["live"] for g in gs)


def _short_cap(pkg, g, n_peers, fn, *lead):
    """The call with room for one entry: (status, count)."""
    off = np.zeros(n_peers + 1, np.uint64)
    one_c, one_h, cnt = np.zeros(1, np.uint64), np.zeros(1, np.uint32), C.c_uint64()
    st = fn(g.h, *lead, n_peers, off.ctypes.data_as(_U64P), one_c.ctypes.data_as(_U64P), one_h.ctypes.data_as(_U32P), 1,
            C.byref(cnt))
    return st, cnt.value


# ---- 1. chain edge shapes ----------------------------------------------------------------------------------

def _chain_subscriptions():
    """Slots 0, 63, 64, 66 (rank 0's last), 67 (rank 1's first), 133, 134 (rank 2's first) and 199: chains of
    1, 2 and 70 (longer than a wavefront), two peers on one slot, the same triple twice."""
    h = [0, 63, 63] + [64] * 70 + [66, 66, 67, 67, 133] + [134] * 70 + [199, 199]
    p = [0, 1, 1] + [i % 4 for i in range(70)] + [0, 3, 2, 2, 4] + [i % 5 for i in range(70)] + [4, 0]
    c = [10, 11, 12] + list(range(100, 170)) + [13, 14, 15, 15, 16] + list(range(200, 270)) + [17, 18]
    return np.array(h, np.uint32), np.array(p, np.uint32), np.array(c, np.uint64)


@pytest.mark.parametrize("labels,path", CODES)
def test_chain_edge_shapes(pkg, gpu_available, labels, path):
    gs, block, n = _chain(pkg, labels, 0)
    _set_path(pkg, gs, path)
    assert block == 67 and n - 2 * block == 66 and all(g.n_handles == 75 for g in gs)
    for g in gs:
        g.snapshot()
    sh, sp, sc = _chain_subscriptions()
    n_peers = 5
    for r, g in enumerate(gs):   # before any wave: nothing
        off, calls, _ = g.part_last_wave_fanout(n_peers)
        assert len(calls) == 0 and not off.any()
    assert not _subscribe_all(pkg, gs, block, sh, sp, sc).any()
    assert _live(gs) == len(sh)
    inv = np.arange(n, dtype=np.uint32)
    pkg.fgi.part_local_invalidate(gs, [0])
    for r, g in enumerate(gs):
        lo, hi = _range(r, block, n)
        want = rank_join(inv, sh, sp, sc, n_peers, lo, hi)
        assert len(want[1]) >= 3
        st, cnt = _short_cap(pkg, g, n_peers, g.lib.fgi_part_last_wave_fanout)
        assert st == pkg.fgi.ECAPACITY and cnt == len(want[1])
        first = g.part_last_wave_fanout(n_peers)
        assert_fanout(first, want, f"root 0, rank {r}")
        assert np.all((first[2] >= lo) & (first[2] < hi)), "slots are not global ids of the rank's range"
        again = g.part_last_wave_fanout(n_peers)
        assert all(np.array_equal(a, b) for a, b in zip(first, again)), "a second call returns other arrays"
        stats = g.sub_stats()
        assert stats["live"] == 0 and stats["delivered"] == len(want[1])
        assert stats["from_list" if path == 1 else "from_bits"] == 1 and stats["from_bits" if path == 1 else "from_list"] == 0
    # one-shot: the same wave again delivers nothing
    for g in gs:
        g.restore()
        off, calls, _ = g.part_last_wave_fanout(n_peers)   # after fgi_restore: no wave's fan-out is left
        assert len(calls) == 0 and not off.any()
    pkg.fgi.part_local_invalidate(gs, [0])
    for g in gs:
        off, calls, _ = g.part_last_wave_fanout(n_peers)
        assert len(calls) == 0 and not off.any()
    # root 134, the first slot of rank 2: ranks 0 and 1 hold entries and launch nothing
    for g in gs:
        g.restore()
    assert not _subscribe_all(pkg, gs, block, sh, sp, sc).any()
    before = [g.sub_stats() for g in gs]
    pkg.fgi.part_local_invalidate(gs, [134])
    inv = np.arange(134, n, dtype=np.uint32)
    for r, g in enumerate(gs):
        got = g.part_last_wave_fanout(n_peers)
        if r < 2:
            assert len(got[1]) == 0 and not got[0].any()
            after = g.sub_stats()
            assert after["fanouts"] == before[r]["fanouts"] and after["live"] == before[r]["live"] > 0
        else:
            want = rank_join(inv, sh, sp, sc, n_peers, *_range(r, block, n))
            assert len(want[1]) == 72
            assert_fanout(got, want, "root 134, rank 2")
    # no roots
    for g in gs:
        g.restore()
    pkg.fgi.part_local_invalidate(gs, [])
    for g in gs:
        off, calls, _ = g.part_last_wave_fanout(n_peers)
        assert len(calls) == 0 and not off.any()
    for g in gs:
        g.close()


# ---- 2. mixed states against the oracle --------------------------------------------------------------------

@pytest.mark.parametrize("labels,path", CODES_AUTO)
@pytest.mark.parametrize("P,direction", [(2, 0), (3, 0), (3, 1), (3, 2), (8, 0)])
def test_three_mixed_waves(pkg, gpu_available, P, direction, labels, path):
    arrays, waves, _ = _mixed()
    sh, sp, sc, dead, live_at, left = mixed_subscriptions()
    assert (int((~dead).sum()), int(dead.sum())) == (5477, 523)
    gs, block = _build_with(pkg, P, N, *arrays, options={pkg.fgi.OPT_PULL_TPB: 1, pkg.fgi.OPT_FANOUT_PATH: path},
                            direction=direction, labels=labels)
    res = _subscribe_all(pkg, gs, block, sh, sp, sc)
    assert np.array_equal(res, np.where(dead, pkg.fgi.SUB_INVALIDATED, pkg.fgi.SUB_ADDED))
    assert _live(gs) == 5477
    for k, (roots, imm, inv, *_rest) in enumerate(waves):
        pkg.fgi.part_local_invalidate(gs, roots, imm)
        m = live_at[k]
        for r, g in enumerate(gs):
            lo, hi = _range(r, block, N)
            want = rank_join(inv, sh[m], sp[m], sc[m], MIXED_PEERS, lo, hi)
            assert len(want[1]) >= 9
            listed = path == 1
            if path == 0 and r % 2 == 0:   # the automatic rule: the list once the rank's ascending ids stand
                assert np.array_equal(g.part_last_wave_ids(), inv[(inv >= lo) & (inv < hi)])
                listed = True
            before = g.sub_stats()
            assert_fanout(g.part_last_wave_fanout(MIXED_PEERS), want, f"wave {k}, rank {r}")
            after = g.sub_stats()
            assert after["from_list"] - before["from_list"] == int(listed)
            assert after["from_bits"] - before["from_bits"] == int(not listed)
    assert _live(gs) == int(left.sum()) > 0
    for g in gs:
        g.close()


# ---- 3. planned waves and small buckets --------------------------------------------------------------------

@pytest.mark.parametrize("labels,path", CODES)
@pytest.mark.parametrize("P", [2, 4])
def test_planned_waves_and_small_buckets(pkg, gpu_available, P, labels, path):
    """The same roots host-driven, planned, planned again, then with buckets of one id per peer, whose wave
    repeats its final collect: the fan-out is the same every time."""
    arrays, waves, _ = _mixed()
    sh, sp, sc, dead, live_at, _ = mixed_subscriptions()
    gs, block = _build_with(pkg, P, N, *arrays, options={pkg.fgi.OPT_PULL_TPB: 1, pkg.fgi.OPT_FANOUT_PATH: path},
                            labels=labels)
    for g in gs:
        g.snapshot()
    roots, imm, inv, *_rest = waves[0]
    m = live_at[0]
    _subscribe_all(pkg, gs, block, sh, sp, sc)
    hit = m & np.isin(sh, inv)
    for what in ("host-driven", "planned", "planned again", "planned, small buckets"):
        if what.endswith("buckets"):
            for g in gs:
                g.set_option(pkg.fgi.OPT_PART_BUCKET, 2)
        print(f"P={P} labels={labels} path={path}: {what}")   # shown if the wave below is refused
        stats = pkg.fgi.part_local_invalidate(gs, roots, imm)
        if what == "planned again":
            assert all(x.host_syncs == 2 for x in stats), [x.host_syncs for x in stats]
        for r, g in enumerate(gs):
            want = rank_join(inv, sh[m], sp[m], sc[m], MIXED_PEERS, *_range(r, block, N))
            assert len(want[1]) >= 9
            assert_fanout(g.part_last_wave_fanout(MIXED_PEERS), want, f"{what}, rank {r}")
        assert _live(gs) == int(m.sum()) - int(hit.sum())
        for g in gs:   # the graph as before the wave, the delivered entries stored again
            g.restore()
        assert not _subscribe_all(pkg, gs, block, sh[hit], sp[hit], sc[hit]).any()
    for g in gs:
        g.close()


# ---- 4. subscribe right after a wave -----------------------------------------------------------------------

@pytest.mark.parametrize("labels,path", CODES)
def test_subscribe_right_after_a_wave(pkg, gpu_available, labels, path):
    """No call between the wave and fgi_part_subscribe: the state is read from the node words and the visit
    bits at the engine's index. An owned slot the wave invalidated completes at once, one that is still
    Consistent is stored, and the wave's ids, bitmap and flagged set are as before the call."""
    arrays, waves, _ = _mixed()
    P = 3
    gs, block = _build_with(pkg, P, N, *arrays, options={pkg.fgi.OPT_PULL_TPB: 1, pkg.fgi.OPT_FANOUT_PATH: path},
                            labels=labels)
    roots, imm, inv, fl_ids, fl, _ = waves[0]
    v1, f1 = _mixed_states()[1]
    consistent = np.flatnonzero((v1[:N] != 0) & ((f1[:N] & 3) == CONSISTENT)).astype(np.uint32)
    pkg.fgi.part_local_invalidate(gs, roots, imm)
    stored = 0
    for r, g in enumerate(gs):
        lo, hi = _range(r, block, N)
        mine = inv[(inv >= lo) & (inv < hi)].astype(np.uint32)
        ok = consistent[(consistent >= lo) & (consistent < hi)]
        assert len(mine) >= 8 and len(ok) >= 8
        sh = np.concatenate([mine[:8], ok[:8], [(hi % N)]]).astype(np.uint32)   # the last one: another rank's
        res = g.part_subscribe(sh, np.zeros(len(sh), np.uint32), np.arange(len(sh), dtype=np.uint64))
        assert res.tolist() == [pkg.fgi.SUB_INVALIDATED] * 8 + [pkg.fgi.SUB_ADDED] * 8 + [pkg.fgi.SUB_NOT_OWNED]
        stored += 8
        # the wave's answers, first asked for after the subscribe, against the oracle
        assert np.array_equal(g.part_last_wave_ids(), mine)
        bits, nb = g.part_last_wave_bits()
        assert nb == len(mine) and np.array_equal(pkg.fgi.bits_to_ids(bits) + np.uint32(lo), mine)
        _, gi, gf = g.part_last_flagged()
        keep = (fl_ids >= lo) & (fl_ids < hi)
        assert np.array_equal(gi, fl_ids[keep]) and np.array_equal(gf, fl[keep])
        # and the same arrays around a second subscribe
        assert g.part_subscribe(ok[8:12], [1] * 4, [100, 101, 102, 103]).tolist() == [pkg.fgi.SUB_ADDED] * 4
        stored += 4
        assert np.array_equal(g.part_last_wave_ids(), mine) and np.array_equal(g.part_last_wave_bits()[0], bits)
        _, gi2, gf2 = g.part_last_flagged()
        assert np.array_equal(gi2, gi) and np.array_equal(gf2, gf)
        # nothing of what was stored is in the wave's set
        off, calls, _ = g.part_last_wave_fanout(2)
        assert len(calls) == 0 and off.tolist() == [0, 0, 0]
    assert _live(gs) == stored
    for g in gs:
        g.close()


# ---- 5. entries follow the node ----------------------------------------------------------------------------

def _small(pkg, labels, path):
    """12 slots over 2 ranks: 0 -> 1 -> 2 on rank 0; slot 9 (rank 1) delayed, without dependants."""
    n, x = 12, 9
    v = O.version_of(3, np.arange(n, dtype=np.uint64)).copy()
    f = np.full(n, CONSISTENT, np.uint32)
    f[x] |= F_HD
    src, dst = np.array([0, 1], np.uint32), np.array([1, 2], np.uint32)
    gs, block = _build_with(pkg, 2, n, v, f, src, dst, v[dst], options={pkg.fgi.OPT_FANOUT_PATH: path}, labels=labels,
                            n_detached=4)
    assert block == 6
    return gs, block, x


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("labels,path", CODES)
def test_entries_follow_the_node(pkg, gpu_available, labels, path, direct):
    """The displacement through a batch's BEGIN_COMPUTE step, and through fgi_part_begin_compute itself (a
    collective: one host thread per rank)."""
    sh, sp, sc = np.array([9, 9, 1], np.uint32), np.array([0, 1, 1], np.uint32), np.array([30, 31, 50], np.uint64)
    for release in (False, True):
        gs, block, x = _small(pkg, labels, path)
        assert not _subscribe_all(pkg, gs, block, sh, sp, sc).any()
        if direct:
            outs = _each_rank(gs, lambda r, g: g.part_begin_compute([x], [(1 << 41) + 1])[0])
            assert int(outs[0][0]) == NONE   # rank 0 does not own x
            d = int(outs[1][0])
            for g in gs:   # a mutation's cascades: through fgi_part_fanout_ids
                with pytest.raises(pkg.FgiError) as e:
                    g.part_last_wave_fanout(2)
                assert e.value.status == pkg.fgi.ENOTSUP and "fgi_part_fanout_ids" in str(e.value)
        else:
            ids, outs, _ = pkg.fgi.part_local_run_batch(gs, [("begin_compute", [x], [(1 << 41) + 1])])
            d = int(outs[0][0])
        assert d != NONE and block <= d < block + 4   # the delayed node lives on, detached
        assert [g.sub_stats()["live"] for g in gs] == [1, 2]
        if release:   # the host gives the displaced node up: its entries are dropped with the handle
            gs[1].release([d])
            st = gs[1].sub_stats()
            assert (st["live"], st["dropped"], st["delivered"]) == (0, 2, 0)
        else:
            # the new node at x becomes Consistent and is invalidated: the entries are not its
            ids, _, _ = pkg.fgi.part_local_run_batch(gs, [("set_output", [x]), ("invalidate", [x], [1])])
            assert x in ids.tolist()
            for g in gs:
                off, calls, _ = g.part_fanout_ids(np.unique(ids), 2)
                assert len(calls) == 0 and off.tolist() == [0, 0, 0]
            # the host ends the displaced node itself: the owner returns its entries by the detached handle
            want = np_join(np.array([d], np.uint32), np.array([d, d], np.uint32), sp[:2], sc[:2], 2)
            assert len(want[1]) == 2
            assert_fanout(gs[1].part_fanout_detached([d], 2), want, "detached")
            off, calls, _ = gs[1].part_fanout_detached([d], 2)   # one-shot
            assert len(calls) == 0
            assert [g.sub_stats()["live"] for g in gs] == [1, 0]
        for g in gs:
            g.close()


# ---- 6. batches --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("labels,path", CODES)
def test_batches(pkg, gpu_available, labels, path):
    gs, block, n = _chain(pkg, labels, 0)
    _set_path(pkg, gs, path)
    sh, sp, sc = _chain_subscriptions()
    n_peers = 5
    assert not _subscribe_all(pkg, gs, block, sh, sp, sc).any()
    ids, _, _ = pkg.fgi.part_local_run_batch(gs, [("invalidate", [100])])
    ids = np.sort(ids)
    assert np.array_equal(ids, np.arange(100, n, dtype=np.uint32))
    for r, g in enumerate(gs):
        with pytest.raises(pkg.FgiError) as e:   # a batch's cascades: through fgi_part_fanout_ids
            g.part_last_wave_fanout(n_peers)
        assert e.value.status == pkg.fgi.ENOTSUP and "fgi_part_fanout_ids" in str(e.value)
        # the whole merged list to every rank: each returns exactly its share
        want = rank_join(ids, sh, sp, sc, n_peers, *_range(r, block, n))
        assert (len(want[1]) > 0) == (r > 0)
        live = g.sub_stats()["live"]
        assert r < 2 or len(want[1]) == 72
        if len(want[1]) > 1:   # a buffer of one entry is short: the count is reported, nothing is removed
            idp = np.ascontiguousarray(ids)
            st, cnt = _short_cap(pkg, g, n_peers, g.lib.fgi_part_fanout_ids, len(idp), idp.ctypes.data_as(_U32P))
            assert st == pkg.fgi.ECAPACITY and cnt == len(want[1]) and g.sub_stats()["live"] == live
        assert_fanout(g.part_fanout_ids(ids, n_peers), want, f"rank {r}")
        assert g.sub_stats()["live"] == live - len(want[1])
    assert _live(gs) == int((sh < 100).sum())
    for g in gs:
        g.close()


# ---- 7. many tiles -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_peers", [257, 4096])
@pytest.mark.parametrize("labels,path", CODES)
def test_many_tiles(pkg, gpu_available, labels, path, n_peers):
    n, roots, inv, sh, sp, sc, _ = _rmat16()
    P = 2
    block = n // P
    gs = [pkg.Graph(block, n_detached=64, rank=r, world=P, labels=labels) for r in range(P)]
    pkg.fgi.part_init_local(gs, n)
    for g in gs:
        g.set_option(pkg.fgi.OPT_FANOUT_PATH, path)
        g.part_synth_rmat(16, 8, RSEED, 0, 0)
    assert not _subscribe_all(pkg, gs, block, sh, sp, sc).any()
    pkg.fgi.part_local_invalidate(gs, roots)
    # part_synth_rmat with the seed builds _rmat16()'s graph: the wave is the oracle's
    assert np.array_equal(np.sort(np.concatenate([g.part_export_ids() for g in gs])), inv)
    for r, g in enumerate(gs):
        want = rank_join(inv, sh, sp, sc, n_peers, *_range(r, block, n))
        assert len(want[1]) > 10000
        assert_fanout(g.part_last_wave_fanout(n_peers), want, f"rank {r}")
    assert _live(gs) == 200000 - int(np.isin(sh, inv).sum())
    for g in gs:
        g.close()


# ---- 8. status codes and cost ------------------------------------------------------------------------------

def test_status_codes(pkg, gpu_available):
    fgi = pkg.fgi
    single = pkg.Graph(64, n_detached=4)
    for fn in (lambda: single.part_subscribe([0], [0], [1]), lambda: single.part_last_wave_fanout(1),
               lambda: single.part_fanout_ids([0], 1), lambda: single.part_fanout_detached([64], 1),
               lambda: single.part_unsubscribe_peer(0)):
        with pytest.raises(pkg.FgiError) as e:
            fn()
        assert e.value.status == fgi.ENOTSUP
    single.close()
    gs, block, n = _chain(pkg, 1, 0)
    for x in gs:
        x.snapshot()
    g = gs[0]
    for args in (([n], [0], [1]), ([0], [4096], [1])):   # a slot past the partition, a peer past the limit
        with pytest.raises(pkg.FgiError) as e:
            g.part_subscribe(*args)
        assert e.value.status == fgi.EINVAL
    assert g.sub_stats() == {k: 0 for k in g.sub_stats()}   # nothing stored, nothing allocated
    assert g.part_subscribe([0, 1, 70], [0, 5, 0], [1, 2, 3]).tolist() == [0, 0, fgi.SUB_NOT_OWNED]
    pkg.fgi.part_local_invalidate(gs, [0])
    with pytest.raises(pkg.FgiError) as e:   # peer 5 is stored: n_peers must exceed it
        g.part_last_wave_fanout(5)
    assert e.value.status == fgi.EINVAL and g.sub_stats()["live"] == 2
    with pytest.raises(pkg.FgiError) as e:
        g.part_fanout_ids([0, 1], 5)
    assert e.value.status == fgi.EINVAL and g.sub_stats()["live"] == 2
    off, calls, slots = g.part_last_wave_fanout(6)
    assert off.tolist() == [0, 1, 1, 1, 1, 1, 2] and calls.tolist() == [1, 2] and slots.tolist() == [0, 1]
    for fn in (lambda: g.part_fanout_ids([2, 2], 6), lambda: g.part_fanout_ids([3, 2], 6), lambda: g.part_fanout_ids([n], 6),
               lambda: g.part_fanout_detached([block + 1, block], 6), lambda: g.part_fanout_detached([0], 6),
               lambda: g.part_fanout_detached([block + 8], 6), lambda: g.part_unsubscribe_peer(4096)):
        with pytest.raises(pkg.FgiError) as e:
            fn()
        assert e.value.status == fgi.EINVAL
    # a rank that never subscribes (its share of the wave holds 67 slots)
    st = gs[1].sub_stats()
    assert st == {k: 0 for k in st}
    assert len(gs[1].part_last_wave_ids()) == 67
    off, calls, _ = gs[1].part_last_wave_fanout(3)
    assert off.tolist() == [0, 0, 0, 0] and len(calls) == 0
    off, calls, _ = gs[1].part_fanout_ids(np.arange(n, dtype=np.uint32), 3)
    assert off.tolist() == [0, 0, 0, 0] and len(calls) == 0
    assert gs[1].part_unsubscribe_peer(1) == 0
    st = gs[1].sub_stats()
    assert st == {k: 0 for k in st}, st
    # a disconnected peer's entries on this rank
    for x in gs:
        x.restore()
    assert g.part_subscribe([5, 6, 7], [2, 3, 2], [7, 8, 9]).tolist() == [0, 0, 0]
    assert g.part_unsubscribe_peer(2) == 2 and g.part_unsubscribe_peer(2) == 0
    st = g.sub_stats()
    assert (st["live"], st["dropped"], st["delivered"]) == (1, 2, 2)
    for x in gs:
        x.close()


@pytest.mark.parametrize("coll", [0, 1])
@pytest.mark.parametrize("labels,path", CODES)
def test_world_one(pkg, gpu_available, labels, path, coll):
    arrays, waves, _ = _mixed()
    sh, sp, sc, dead, live_at, _ = mixed_subscriptions()
    gs, block = _build_with(pkg, 1, N, *arrays, options={pkg.fgi.OPT_PART_COLLECTIVES: coll, pkg.fgi.OPT_FANOUT_PATH: path},
                            labels=labels)
    g = gs[0]
    res = g.part_subscribe(sh, sp, sc)
    assert np.array_equal(res, dead.astype(np.uint32))
    for k, (roots, imm, inv, *_rest) in enumerate(waves[:2]):
        g.part_invalidate_host(roots, imm, want=None)
        m = live_at[k]
        want = np_join(inv, sh[m], sp[m], sc[m], MIXED_PEERS)
        assert len(want[1]) > 100
        assert_fanout(g.part_last_wave_fanout(MIXED_PEERS), want, f"wave {k}")
    g.close()
