"""The replica fan-out on the device (fgi_subscribe, fgi_last_wave_fanout, fgi_fanout_ids, fgi_unsubscribe_peer,
fgi_sub_stats_get) against a numpy join.

Expected lists are never taken from the engine: they are the test's own subscription arrays joined in numpy
with the invalidated set the CPU oracle gives for the same wave. Both sides are then sorted within their
(peer, handle) runs (the order inside a run is unspecified); that the engine's handles ascend within every
peer is asserted before the sort. Every case runs with the fan-out's source pinned to the id list (1) and to
the bitmap (2), with and without hub-first labels."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import fgo as O
from harness import CONSISTENT, F_HD, INVALIDATED
from test_gpu_count_only import count_only
from test_gpu_flagged import N as MIXED_N, N_DET as MIXED_DET, _engine, _mixed

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NONE = 0xFFFFFFFF
_U32P, _U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
PATHS = [1, 2]
LABELS = [-1, 1]


def np_join(inv, sh, sp, sc, n_peers):
    """(peer_off, call_ids, handles) of the entries (sh, sp, sc) whose handle is in inv: by peer, then handle,
    then call id."""
    keep = np.isin(sh, inv)
    h, p, c = sh[keep], sp[keep], sc[keep]
    order = np.lexsort((c, h, p))
    off = np.zeros(n_peers + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(p, minlength=n_peers))
    return off, c[order].astype(np.uint64), h[order].astype(np.uint32)


def canon(off, calls, hnd):
    """The engine's result with the peer_off invariants and the handle order checked, sorted inside its
    (peer, handle) runs."""
    assert off[0] == 0 and np.all(np.diff(off.astype(np.int64)) >= 0) and off[-1] == len(calls) == len(hnd)
    peer = np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
    same_peer = np.diff(peer) == 0
    assert np.all(np.diff(hnd.astype(np.int64))[same_peer] >= 0), "handles do not ascend within a peer"
    order = np.lexsort((calls, hnd, peer))
    return off, calls[order], hnd[order]


def assert_fanout(got, want, what=""):
    off, calls, hnd = canon(*got)
    assert np.array_equal(off, want[0]), f"{what}: peer_off differs"
    assert np.array_equal(hnd, want[2]), f"{what}: handles differ"
    assert np.array_equal(calls, want[1]), f"{what}: call ids differ"


def wave(g, roots, imm, path):
    """A wave that leaves what the pinned path reads first: its id list (1) or only its kept bitmap (2)."""
    if path == 1:
        return len(g.invalidate(roots, imm))
    return count_only(g, roots, imm)


def oracle_wave(o, roots, imm=None):
    o.clear_log()
    o.invalidate_slots(roots, imm)
    return np.sort(o.inv_log()).astype(np.uint32)


# ---- the golden fixtures ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture(name):
    """The fixture's arrays with one slot without dependants made a delayed Consistent node (x: it survives a
    displacement), and the oracle's invalidated set of the fixture's wave after a computation began on x."""
    doc = json.load(open(os.path.join(GOLDEN, name + ".json")))
    n = doc["n_slots"]
    v = np.array(doc["versions"], np.uint64)
    f = np.array(doc["state_flags"], np.uint32)
    used, dep, tags = (np.array(doc[k], t) for k, t in (("used", np.uint32), ("dependant", np.uint32), ("tags", np.uint64)))
    roots, imm = np.array(doc["roots"], np.uint32), np.array(doc["immediately"], np.uint8)
    free = np.setdiff1d(np.nonzero(v)[0], np.concatenate([used, roots]))
    x = int(free[-1])
    f[x] = CONSISTENT | F_HD
    o = O.Oracle(n)
    o.load_graph(v, f, used, dep, tags)
    xver = np.array([(1 << 40) + 1], np.uint64)
    o.begin_compute_slots(np.array([x], np.uint32), xver, None)
    inv = oracle_wave(o, roots, imm)
    o.close()
    for a in (v, f, used, dep, tags, roots, imm, inv):
        a.setflags(write=False)
    return n, v, f, used, dep, tags, roots, imm, x, xver, inv


def _subscriptions(n, x, n_peers, inv):
    """Entries on handles 0, 63, 64, the last slot and x; chains of 1, 2 and 70 (longer than a wavefront);
    two peers on one handle; the same triple twice; 300 more over all slots. Peers 0 .. min(n_peers, 7) - 1
    and the last peer."""
    rng = np.random.default_rng(n * 31 + n_peers)
    k = min(n_peers, 7)
    mid = int(inv[len(inv) // 2])   # invalidated by the fixture's wave, whatever becomes of handle 64
    h = [0, 63, 63, n - 1, n - 1] + [64] * 70 + [mid] * 70 + [x, x] + [int(inv[0])] * 2
    p = [0, 0, k - 1, 1 % k, 1 % k] + 2 * [i % k for i in range(70)] + [0, n_peers - 1] + [n_peers - 1, 2 % k]
    c = [10, 11, 12, 13, 13] + list(range(100, 240)) + [20, 21, 22, 23]
    h += rng.integers(0, n, 300).tolist()
    p += rng.integers(0, k, 300).tolist()
    c += (1000 + rng.integers(0, 1 << 40, 300)).tolist()
    return np.array(h, np.uint32), np.array(p, np.uint32), np.array(c, np.uint64)


@pytest.mark.parametrize("n_peers", [1, 3, 100, 4096])
@pytest.mark.parametrize("labels", LABELS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["layered_7x40_f4", "mixed_states_imm"])
def test_fixture(pkg, gpu_available, name, path, labels, n_peers):
    n, v, f, used, dep, tags, roots, imm, x, xver, inv = _fixture(name)
    g = _engine(pkg, n, v, f, used, dep, tags, labels=labels, n_detached=5)   # 285 / 305 handles: no multiple of 64
    g.set_option(pkg.fgi.OPT_FANOUT_PATH, path)
    sh, sp, sc = _subscriptions(n, x, n_peers, inv)
    res = g.subscribe(sh, sp, sc)
    # an entry on an empty or Invalidated handle completes at once and is not stored
    dead = (v[sh] == 0) | ((f[sh] & 3) == INVALIDATED)
    assert np.array_equal(res, dead.astype(np.uint32))
    sh, sp, sc = sh[~dead], sp[~dead], sc[~dead]
    assert g.sub_stats()["live"] == len(sh)
    # a computation begins on x: its delayed node lives on at a detached handle and takes its entries along
    d = int(g.begin_compute([x], xver)[0])
    assert d != NONE and d >= n
    sh = np.where(sh == x, d, sh).astype(np.uint32)
    off, calls, hnd = g.last_wave_fanout(n_peers)   # the displacement invalidated nothing
    assert len(calls) == 0 and not off.any()
    # the fixture's wave
    assert wave(g, roots, imm, path) == len(inv)
    want = np_join(inv, sh, sp, sc, n_peers)
    assert len(want[1]) > 70
    # a short buffer reports the count and removes nothing twice
    poff = np.zeros(n_peers + 1, np.uint64)
    one_c, one_h, cnt = np.zeros(1, np.uint64), np.zeros(1, np.uint32), C.c_uint64()
    st = g.lib.fgi_last_wave_fanout(g.h, n_peers, poff.ctypes.data_as(_U64P), one_c.ctypes.data_as(_U64P),
                                    one_h.ctypes.data_as(_U32P), 1, C.byref(cnt))
    assert st == pkg.fgi.ECAPACITY and cnt.value == len(want[1])
    first = g.last_wave_fanout(n_peers)
    assert_fanout(first, want, "wave")
    again = g.last_wave_fanout(n_peers)
    assert all(np.array_equal(a, b) for a, b in zip(first, again)), "a second call returns other arrays"
    if n_peers >= 100:   # peers without entries have empty ranges
        assert first[0][50] == first[0][51]
    left = ~np.isin(sh, inv)
    stats = g.sub_stats()
    assert stats["live"] == int(left.sum()) and stats["delivered"] == len(want[1])
    assert stats["from_list" if path == 1 else "from_bits"] >= 1 and stats["from_bits" if path == 1 else "from_list"] == 0
    # the displaced node (no dependants) is invalidated at its detached handle: x's entries fire there
    assert g.invalidate([d], [1]).tolist() == [d]
    sh, sp, sc = sh[left], sp[left], sc[left]
    want = np_join(np.array([d], np.uint32), sh, sp, sc, n_peers)
    assert len(want[1]) >= 2 and set(want[2].tolist()) == {d}
    assert_fanout(g.last_wave_fanout(n_peers), want, "detached")
    assert g.sub_stats()["live"] == int((sh != d).sum())
    g.close()


# ---- one-shot -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", LABELS)
@pytest.mark.parametrize("path", PATHS)
def test_one_shot_and_pool_reuse(pkg, gpu_available, path, labels):
    n, v, f, used, dep, tags, roots, imm, x, xver, _ = _fixture("layered_7x40_f4")
    o = O.Oracle(n)
    o.load_graph(v, f, used, dep, tags)
    inv = oracle_wave(o, roots, imm)
    o.close()
    g = _engine(pkg, n, v, f, used, dep, tags, labels=labels, n_detached=5)
    g.set_option(pkg.fgi.OPT_FANOUT_PATH, path)
    g.snapshot()
    rng = np.random.default_rng(5)
    sh = rng.choice(inv, 1000).astype(np.uint32)
    sp = rng.integers(0, 9, 1000).astype(np.uint32)
    sc = np.arange(1000, dtype=np.uint64)
    assert not g.subscribe(sh, sp, sc).any()
    pool0 = g.sub_stats()["pool"]
    assert 1000 <= pool0 < 3000
    assert wave(g, roots, imm, path) == len(inv)
    assert_fanout(g.last_wave_fanout(9), np_join(inv, sh, sp, sc, 9), "first")
    assert g.sub_stats()["live"] == 0
    # the table outlives fgi_restore, the delivered entries do not come back
    g.restore()
    assert wave(g, roots, imm, path) == len(inv)
    off, calls, _ = g.last_wave_fanout(9)
    assert len(calls) == 0 and not off.any()
    # 3,000 more: the 1,000 freed records are taken again, so the pool grows once, to less than 4,000
    g.restore()
    sh3 = rng.choice(inv, 3000).astype(np.uint32)
    sp3 = rng.integers(0, 9, 3000).astype(np.uint32)
    sc3 = np.arange(5000, 8000, dtype=np.uint64)
    assert not g.subscribe(sh3, sp3, sc3).any()
    st = g.sub_stats()
    assert st["live"] == 3000 and 3000 <= st["pool"] < 4000 and st["pool"] > pool0
    # after fgi_restore no wave's fan-out is left to make: nothing is delivered, nothing leaves the table
    off, calls, _ = g.last_wave_fanout(9)
    assert len(calls) == 0 and not off.any() and g.sub_stats()["live"] == 3000
    assert wave(g, roots, imm, path) == len(inv)
    assert_fanout(g.last_wave_fanout(9), np_join(inv, sh3, sp3, sc3, 9), "second")
    st = g.sub_stats()
    assert st["live"] == 0 and st["delivered"] + st["dropped"] + st["live"] == 4000
    g.close()


# ---- fgi_subscribe right after a wave -----------------------------------------------------------------------
@pytest.mark.parametrize("labels", LABELS)
@pytest.mark.parametrize("path", PATHS)
def test_subscribe_right_after_a_wave(pkg, gpu_available, path, labels):
    """No call between the wave and fgi_subscribe: the state is read from the node words and the visit bits.
    A handle the wave invalidated completes at once, one it only flagged (a delayed node, a Computing one) is
    stored, and the wave's id list and flagged set are still there afterwards."""
    arrays, waves, _ = _mixed()
    roots, imm, inv, fl_ids, fl, _ = waves[0]
    g = _engine(pkg, MIXED_N, *arrays, labels=labels, n_detached=MIXED_DET)
    g.set_option(pkg.fgi.OPT_FANOUT_PATH, path)
    assert wave(g, roots, imm, path) == len(inv)
    delayed = fl_ids[((fl & 3) == CONSISTENT)]
    assert len(delayed) >= 5 and len(inv) >= 10
    sh = np.concatenate([inv[:10], fl_ids]).astype(np.uint32)
    res = g.subscribe(sh, np.zeros(len(sh), np.uint32), np.arange(len(sh), dtype=np.uint64))
    assert res[:10].tolist() == [1] * 10 and not res[10:].any()
    assert np.array_equal(g.last_wave_ids(), inv)
    gi, gf = g.last_wave_flagged()
    assert np.array_equal(gi, fl_ids) and np.array_equal(gf, fl)
    assert g.sub_stats()["live"] == len(fl_ids)
    # nothing of what was stored is in the wave's set
    off, calls, _ = g.last_wave_fanout(1)
    assert len(calls) == 0 and off.tolist() == [0, 0]
    g.close()


# ---- entries follow the node --------------------------------------------------------------------------------
def _chain6(pkg, labels, path):
    """0 -> 1 -> 2 -> 3 -> 4, node 3 delayed; 5 alone."""
    n = 6
    v = O.version_of(3, np.arange(n, dtype=np.uint64)).copy()
    f = np.full(n, CONSISTENT, np.uint32)
    f[3] |= F_HD
    src, dst = np.array([0, 1, 2, 3], np.uint32), np.array([1, 2, 3, 4], np.uint32)
    g = _engine(pkg, n, v, f, src, dst, v[dst], labels=labels, n_detached=4)
    g.set_option(pkg.fgi.OPT_FANOUT_PATH, path)
    return g


@pytest.mark.parametrize("labels", LABELS)
@pytest.mark.parametrize("path", PATHS)
def test_entries_follow_the_node(pkg, gpu_available, path, labels):
    g = _chain6(pkg, labels, path)
    assert not g.subscribe([3, 3, 5], [0, 1, 1], [30, 31, 50]).any()
    d = int(g.begin_compute([3], [(1 << 41) + 1])[0])
    assert d >= 6 and d != NONE
    # the new node at slot 3 becomes Consistent and is invalidated: the entries are not its
    g.set_output([3])
    assert wave(g, [3], None, path) == 1
    off, calls, _ = g.last_wave_fanout(2)
    assert len(calls) == 0
    # the displaced node, invalidated at once at its detached handle
    assert wave(g, [d], [1], path) >= 1
    assert_fanout(g.last_wave_fanout(2), np_join(np.array([d]), np.array([d, d, 5], np.uint32), np.array([0, 1, 1]),
                                                 np.array([30, 31, 50], np.uint64), 2), "detached")
    st = g.sub_stats()
    assert (st["live"], st["delivered"]) == (1, 2)
    g.close()


@pytest.mark.parametrize("labels", LABELS)
@pytest.mark.parametrize("path", PATHS)
def test_entries_follow_the_node_through_a_batch(pkg, gpu_available, path, labels):
    """Two BEGIN_COMPUTE steps on slot 3 in one batch: the entries go with the first displaced node (the
    delayed one), not with the Computing node the second step displaces."""
    g = _chain6(pkg, labels, path)
    assert not g.subscribe([3, 3], [0, 1], [30, 31]).any()
    _, outs = g.run_batch([("begin_compute", [3], [(1 << 41) + 1]), ("begin_compute", [3], [(1 << 41) + 3])])
    d1, d2 = int(outs[0][0]), int(outs[1][0])
    assert NONE not in (d1, d2) and d1 != d2
    with pytest.raises(pkg.FgiError) as e:   # a batch's cascades: through fgi_fanout_ids
        g.last_wave_fanout(2)
    assert e.value.status == pkg.fgi.ENOTSUP and "fgi_fanout_ids" in str(e.value)
    ids, _ = g.run_batch([("invalidate", [d2], [1])])
    off, calls, _ = g.fanout_ids(np.unique(ids), 2)
    assert len(calls) == 0 and off.tolist() == [0, 0, 0]
    ids, _ = g.run_batch([("invalidate", [d1], [1])])
    assert d1 in ids.tolist()
    want = np_join(np.array([d1]), np.array([d1, d1], np.uint32), np.array([0, 1]), np.array([30, 31], np.uint64), 2)
    assert_fanout(g.fanout_ids(np.unique(ids), 2), want, "batch")
    assert g.sub_stats()["live"] == 0
    g.close()


@pytest.mark.parametrize("path", PATHS)
def test_release_and_unsubscribe_peer(pkg, gpu_available, path):
    g = _chain6(pkg, -1, path)
    assert not g.subscribe([3, 3, 3, 0, 0, 5], [0, 1, 2, 1, 2, 1], [30, 31, 32, 1, 2, 50]).any()
    d = int(g.begin_compute([3], [(1 << 41) + 1])[0])
    g.release([d])   # the released handle's three entries go with it
    st = g.sub_stats()
    assert (st["live"], st["dropped"]) == (3, 3)
    assert g.unsubscribe_peer(1) == 2   # (0, 1, 1) and (5, 1, 50)
    assert g.unsubscribe_peer(1) == 0
    st = g.sub_stats()
    assert (st["live"], st["dropped"]) == (1, 5)
    assert wave(g, [0, 5], None, path) >= 2
    want = np_join(np.array([0]), np.array([0], np.uint32), np.array([2]), np.array([2], np.uint64), 3)
    assert_fanout(g.last_wave_fanout(3), want, "after the drops")
    st = g.sub_stats()
    assert st["live"] == 0 and st["delivered"] + st["dropped"] == 6
    g.close()


# ---- status codes -------------------------------------------------------------------------------------------
def test_status_codes(pkg, gpu_available):
    fgi = pkg.fgi
    g = _chain6(pkg, -1, 0)
    for args in (([6 + 4], [0], [1]), ([0], [4096], [1])):   # a handle past the detached ones, a peer past the limit
        with pytest.raises(pkg.FgiError) as e:
            g.subscribe(*args)
        assert e.value.status == fgi.EINVAL
    assert g.sub_stats() == {k: 0 for k in g.sub_stats()}   # nothing stored, nothing allocated
    assert not g.subscribe([0, 1], [0, 5], [1, 2]).any()
    g.invalidate([0])
    with pytest.raises(pkg.FgiError) as e:   # peer 5 is stored: n_peers must exceed it
        g.last_wave_fanout(5)
    assert e.value.status == fgi.EINVAL and g.sub_stats()["live"] == 2
    off, calls, hnd = g.last_wave_fanout(6)
    assert off.tolist() == [0, 1, 1, 1, 1, 1, 2] and calls.tolist() == [1, 2] and hnd.tolist() == [0, 1]
    with pytest.raises(pkg.FgiError) as e:   # not strictly ascending
        g.fanout_ids([2, 2], 6)
    assert e.value.status == fgi.EINVAL
    # after an asynchronous ticket
    g2 = _chain6(pkg, -1, 0)
    assert not g2.subscribe([1], [0], [7]).any()
    t = g2.invalidate_async_host([0])
    with pytest.raises(pkg.FgiError) as e:
        g2.last_wave_fanout(1)
    assert e.value.status == fgi.ENOTSUP and "fgi_fanout_ids" in str(e.value)
    off, calls, hnd = g2.fanout_ids(g2.wave_wait_ids(t), 1)
    assert calls.tolist() == [7] and hnd.tolist() == [1]
    g.close()
    g2.close()
    # a partition (two ranks in one process)
    gs = [pkg.Graph(32, rank=r, world=2) for r in range(2)]
    fgi.part_init_local(gs, 64)
    for fn in (lambda: gs[0].subscribe([0], [0], [1]), lambda: gs[0].last_wave_fanout(1),
               lambda: gs[0].fanout_ids([0], 1), lambda: gs[0].unsubscribe_peer(0)):
        with pytest.raises(pkg.FgiError) as e:
            fn()
        assert e.value.status == fgi.ENOTSUP
    for x in gs:
        x.close()


# ---- many tiles ---------------------------------------------------------------------------------------------
RSEED = 0x5EED0F09


@functools.lru_cache(maxsize=None)
def _rmat16():
    scale = 16
    n = 1 << scale
    s, d = O.gen_rmat(scale, 8, RSEED)
    roots = O.gen_roots(512, n, 0x5EED1F0A, np.bincount(s, minlength=n))
    o = O.Oracle(n)
    o.load_graph(O.version_of(RSEED, np.arange(n)), None, s, d, O.gen_tags(s, d, RSEED))
    inv = oracle_wave(o, roots)
    o.close()
    rng = np.random.default_rng(16)
    sh = rng.integers(0, n, 200000).astype(np.uint32)
    sp = rng.integers(0, 257, 200000).astype(np.uint32)
    sc = rng.integers(0, 1 << 62, 200000).astype(np.uint64)
    want = {p: np_join(inv, sh, sp, sc, p) for p in (257, 4096)}
    for a in (roots, inv, sh, sp, sc):
        a.setflags(write=False)
    return n, roots, inv, sh, sp, sc, want


@pytest.mark.parametrize("n_peers", [257, 4096])   # 4,096 peers: the tile table's size limit makes tiles of two words
@pytest.mark.parametrize("labels", LABELS)
@pytest.mark.parametrize("path", PATHS)
def test_many_tiles(pkg, gpu_available, path, labels, n_peers):
    n, roots, inv, sh, sp, sc, want = _rmat16()
    assert len(inv) > 10000 and len(want[n_peers][1]) > 30000
    g = pkg.Graph(n, n_detached=64, labels=labels)
    g.synth_rmat(16, 8, RSEED, 0, 0)
    g.set_option(pkg.fgi.OPT_FANOUT_PATH, path)
    g.snapshot()
    assert not g.subscribe(sh, sp, sc).any()
    assert wave(g, roots, None, path) == len(inv)
    assert_fanout(g.last_wave_fanout(n_peers), want[n_peers], "last_wave_fanout")
    assert g.sub_stats()["live"] == 200000 - len(want[n_peers][1])
    # the same join from the wave's own ids, the delivered entries subscribed again
    g.restore()
    back = np.isin(sh, inv)
    assert not g.subscribe(sh[back], sp[back], sc[back]).any()
    ids = g.invalidate(roots)
    assert np.array_equal(ids, inv)
    assert_fanout(g.fanout_ids(ids, n_peers), want[n_peers], "fanout_ids")
    assert g.sub_stats()["live"] == 200000 - len(want[n_peers][1])
    g.close()


# ---- no subscriptions ---------------------------------------------------------------------------------------
def test_no_subscriptions_cost_nothing(pkg, gpu_available):
    doc = json.load(open(os.path.join(GOLDEN, "layered_7x40_f4.json")))
    n, v, f, used, dep, tags, roots, imm, *_ = _fixture("layered_7x40_f4")
    v0, f0 = np.array(doc["versions"], np.uint64), np.array(doc["state_flags"], np.uint32)
    g = _engine(pkg, n, v0, f0, used, dep, tags, n_detached=5)
    ws = pkg.WaveStats()
    ids = g.invalidate(roots, imm, stats=ws)
    assert sorted(ids.tolist()) == doc["expected"]["inv"]
    assert (ws.v_inv, ws.e_trav) == (doc["expected"]["v_inv"], doc["expected"]["e_trav"])
    off, calls, hnd = g.last_wave_fanout(3)
    assert off.tolist() == [0, 0, 0, 0] and len(calls) == len(hnd) == 0
    off, calls, hnd = g.fanout_ids(ids, 3)
    assert off.tolist() == [0, 0, 0, 0] and len(calls) == 0
    assert g.unsubscribe_peer(1) == 0
    st = g.sub_stats()
    assert st == {k: 0 for k in st}, st
    g.close()
    # and a graph that does subscribe runs the same wave: every statistic but the timings is equal
    g2 = _engine(pkg, n, v0, f0, used, dep, tags, n_detached=5)
    live = np.nonzero(v0)[0].astype(np.uint32)
    g2.subscribe(live, live % 3, live.astype(np.uint64))
    ws2 = pkg.WaveStats()
    assert np.array_equal(g2.invalidate(roots, imm, stats=ws2), ids)
    a, b = ws.as_dict(), ws2.as_dict()
    assert {k: x for k, x in a.items() if not k.endswith("_ms")} == {k: x for k, x in b.items() if not k.endswith("_ms")}
    g2.close()
