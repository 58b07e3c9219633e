"""Count-only synchronous waves against the CPU oracle.

A call that hands no ids back (fgi_invalidate without out_ids, fgi_invalidate_dev without out_ids_dev,
fgi_invalidate_bits) runs no list kernel: the wave ends in the count kernel, which leaves the wave state
clean but for the invalidated bitmap. That bitmap is kept until the next wave starts (the list on demand,
the bits download and the hot labels' folded bitmap read it); the next synchronous wave swaps in the clean
second bitmap and its end kernel clears the kept one. Checked here: the counts, the node states, the list
made on demand, no stale bit from either bitmap across consecutive waves, and every hand-over between a
count-only wave and the other drivers (list-returning, bits, asynchronous, batch cascades, mutations, the
pruner), on graphs whose handle counts straddle the bitmap's word boundary, on R-MAT graphs with and
without hub-first labels (one, two and three fold tiles) in every direction, and on the mixed-state graph
whose waves flag nodes and feed a state view (such graphs keep their bitmap and start with the init
kernel)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fgo as O
from harness import CONSISTENT, assert_states_equal
from test_gpu_flagged import N as MIXED_N, N_DET as MIXED_DET, _dump_handles, _engine, _mixed, _oracle
from test_gpu_state_view import assert_view

pytestmark = pytest.mark.gpu

_U32P = C.POINTER(C.c_uint32)
_U8P = C.POINTER(C.c_uint8)


def count_only(g, roots, imm=None, stats=None):
    """fgi_invalidate without an id destination: the count alone."""
    r = np.ascontiguousarray(np.asarray(roots, np.uint32))
    i = None if imm is None else np.ascontiguousarray(np.asarray(imm, np.uint8))
    n = C.c_uint64()
    st = g.lib.fgi_invalidate(g.h, len(r), r.ctypes.data_as(_U32P), None if i is None else i.ctypes.data_as(_U8P),
                              None, 0, C.byref(n), C.byref(stats) if stats is not None else None)
    g._check(st, "invalidate (count only)")
    return n.value


def oracle_wave(o, roots, imm=None):
    o.clear_log()
    st = o.invalidate_slots(roots, imm)
    return np.sort(o.inv_log()), st


# ---- bitmap word boundaries ----------------------------------------------------------------------------
def _small(pkg, n, kind, n_det):
    versions = O.version_of(11, np.arange(n, dtype=np.uint64)).copy()
    flags = np.full(n, CONSISTENT, np.uint32)
    if kind == "chain":
        src, dst = np.arange(n - 1, dtype=np.uint32), np.arange(1, n, dtype=np.uint32)
    else:
        src, dst = np.zeros(n - 1, np.uint32), np.arange(1, n, dtype=np.uint32)
    tags = versions[dst]
    g = pkg.Graph(n, n_detached=n_det)
    g.register_nodes(np.arange(n, dtype=np.uint32), versions, flags)
    g.load_edges(src, dst, tags)
    o = O.Oracle(n)
    o.load_graph(versions, flags, src, dst, tags)
    return g, o


@pytest.mark.parametrize("n_det", [0, 64])
@pytest.mark.parametrize("kind", ["chain", "fan"])
@pytest.mark.parametrize("n", [40, 63, 64, 65])
def test_word_boundaries(pkg, gpu_available, n, kind, n_det):
    """Two count-only waves (the second starts from the kept state: the swap), the last handle among the
    roots; the list on demand after each, then a third wave behind the list (the full-init path)."""
    g, o = _small(pkg, n, kind, n_det)
    g.snapshot()
    o.snapshot()
    for roots in ([n - 1], [n // 2, n - 2], [0]):
        want, st = oracle_wave(o, roots)
        assert count_only(g, roots) == len(want) == st.v_inv
        if roots != [n - 1]:   # the first wave's list is never asked for: its bitmap must not leak into the next
            assert np.array_equal(g.last_wave_ids(), want)
    assert_states_equal(g, o, n)
    # the bench's shape on the same graph: restore, count, nothing else
    for _ in range(3):
        g.restore()
        o.restore()
        want, _ = oracle_wave(o, [0])
        assert count_only(g, [0]) == len(want) == n
    assert np.array_equal(g.last_wave_ids(), want)
    assert_states_equal(g, o, n)


def test_deep_chain_ends_more_than_once(pkg, gpu_available):
    """A fresh graph's first level group holds four levels: the 40-node chain's first wave needs more, so
    the end kernel runs once per group within one wave (it clears the wave state only with the last).
    warm: a count-only wave of one node comes first, so the deep wave starts by swapping the bitmaps."""
    n = 40
    for warm in (False, True):
        g, o = _small(pkg, n, "chain", 0)
        if warm:
            oracle_wave(o, [n - 1])
            assert count_only(g, [n - 1]) == 1
        ws = pkg.WaveStats()
        want, st = oracle_wave(o, [0])
        assert count_only(g, [0], stats=ws) == len(want) == n - warm
        assert ws.host_syncs > 1, ws.host_syncs
        assert ws.v_inv == st.v_inv
        if not warm:
            assert ws.e_trav == st.e_trav
        assert np.array_equal(g.last_wave_ids(), want)
        assert_states_equal(g, o, n)
        # and a further wave: nothing left to invalidate, nothing stale
        assert count_only(g, [0]) == 0
        assert len(g.last_wave_ids()) == 0


# ---- R-MAT ---------------------------------------------------------------------------------------------
RSEED = 0x5EED0C01


@functools.lru_cache(maxsize=None)
def _rmat_edges(scale):
    s, d = O.gen_rmat(scale, 8, RSEED)
    n = 1 << scale
    deg = np.bincount(s, minlength=n)
    # three disjoint root batches. One node with a dependant reaches most of what can be reached, so: A is
    # nodes without dependants (a wide wave of one level), B is more of those plus eight nodes of one or two
    # dependants (the deep wave), C is hubs (after A and B little is left; fresh, another deep wave).
    rng = np.random.default_rng(scale)
    leaves = rng.permutation(np.nonzero(deg == 0)[0]).astype(np.uint32)
    k = min(len(leaves) // 3, 1500)
    a = np.sort(leaves[:k])
    low = rng.permutation(np.nonzero((deg > 0) & (deg <= 2))[0]).astype(np.uint32)[:8]
    b = np.sort(np.concatenate([leaves[k:k + k // 2], low]))
    c = np.setdiff1d(O.gen_roots(64, n, 0x5EED1C03, deg), np.concatenate([a, b]))
    for r in (s, d, a, b, c):
        r.setflags(write=False)
    return s, d, (a, b, c)


def _rmat_pair(pkg, scale, labels, direction=0, n_det=64):
    s, d, batches = _rmat_edges(scale)
    n = 1 << scale
    g = pkg.Graph(n, n_detached=n_det, labels=labels)
    g.synth_rmat(scale, 8, RSEED, 0, 0)
    g.set_option(pkg.fgi.OPT_DIRECTION, direction)
    o = O.Oracle(n)
    o.load_graph(O.version_of(RSEED, np.arange(n)), None, s, d, O.gen_tags(s, d, RSEED))
    return g, o, batches


@pytest.mark.parametrize("mode", ["plain", "restore", "ids_after_b"])
@pytest.mark.parametrize("direction", [0, 1, 2])
@pytest.mark.parametrize("labels", [-1, 1])
def test_rmat_three_waves_no_stale_bits(pkg, gpu_available, labels, direction, mode):
    """Three consecutive count-only waves A, B, C from disjoint root batches. plain: no restore and no ids
    request in between; restore: fgi_restore before each wave; ids_after_b: the list asked for after B (the
    on-demand list dirties the counters: C starts with the init kernel). After C the list on demand is the
    oracle's C set exactly — nothing of A's, whose bitmap B's end cleared, nothing of B's."""
    scale = 15
    n = 1 << scale
    g, o, batches = _rmat_pair(pkg, scale, labels, direction)
    g.snapshot()
    o.snapshot()
    want, sizes = None, []
    for k, roots in enumerate(batches):
        if mode == "restore":
            g.restore()
            o.restore()
        want, st = oracle_wave(o, roots)
        ws = pkg.WaveStats()
        assert count_only(g, roots, stats=ws) == len(want), f"wave {k}"
        assert ws.v_inv == st.v_inv
        sizes.append(len(want))
        if mode == "ids_after_b" and k == 1:
            assert np.array_equal(g.last_wave_ids(), want)
    # not vacuous (the oracle alone gives 1,500 / 17,786 / 14 without restores, 1,500 / 18,130 / 17,550 with)
    assert sizes[0] > 1000 and sizes[1] > 10000 and sizes[2] > 0, sizes
    assert np.array_equal(g.last_wave_ids(), want)
    assert_states_equal(g, o, n)
    o.close()
    g.close()


def test_rmat17_labelled_three_fold_tiles(pkg, gpu_available):
    """131,072 + 64 handles: three fold tiles, so the labelled end kernel's tile loop runs and the folded
    bitmap (the bits download's source) is written by a count-only end."""
    scale = 17
    n = 1 << scale
    g, o, (a, b, c) = _rmat_pair(pkg, scale, 1)
    want_a, _ = oracle_wave(o, a)
    assert count_only(g, a) == len(want_a)
    want_b, _ = oracle_wave(o, b)
    bits, nb = g.invalidate_bits(b)
    assert nb == len(want_b) and np.array_equal(pkg.fgi.bits_to_ids(bits), want_b)
    want_c, _ = oracle_wave(o, c)
    assert count_only(g, c) == len(want_c)
    assert np.array_equal(g.last_wave_ids(), want_c)
    assert_states_equal(g, o, n)
    o.close()
    g.close()


# ---- repeats as the bench does -------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [-1, 1])
def test_repeats_as_the_bench(pkg, gpu_available, labels):
    import torch
    scale = 15
    n = 1 << scale
    g, o, (_, roots, _) = _rmat_pair(pkg, scale, labels)
    twin, _, _ = _rmat_pair(pkg, scale, labels)
    tw = pkg.WaveStats()
    twin_ids = twin.invalidate(roots, stats=tw)
    want, st = oracle_wave(o, roots)
    assert np.array_equal(twin_ids, want)
    d_roots = torch.from_numpy(roots.astype(np.int32)).cuda()
    g.snapshot()
    # as the bench: a first wave and warm-up steps come before the repeats that are looked at. The first wave
    # runs push-only until a level group has shown a frontier heavy enough to build the dependency lists, and
    # the second is the first to pull, so each sizes its level groups from a wave of another shape: two
    # synchronisations each, with the list kernel and without it alike; from the third wave on it is one.
    for _ in range(2):
        g.restore()
        assert g.invalidate_dev(len(roots), d_roots.data_ptr(), 0, pkg.WaveStats()) == len(want)
    for rep in range(3):
        g.restore()
        ws = pkg.WaveStats()
        assert g.invalidate_dev(len(roots), d_roots.data_ptr(), 0, ws) == len(want)
        assert (ws.v_inv, ws.e_trav, ws.levels) == (tw.v_inv, tw.e_trav, tw.levels), rep
        assert ws.e_trav == st.e_trav
        assert ws.host_syncs == 1, (rep, ws.host_syncs)
        if rep != 1:
            assert np.array_equal(g.last_wave_ids(), want), rep
    assert_states_equal(g, o, n)
    o.close()
    g.close()
    twin.close()


# ---- interleavings -------------------------------------------------------------------------------------
def _after_list(pkg, g, o, b):
    want, _ = oracle_wave(o, b)
    assert np.array_equal(g.invalidate(b), want)


def _after_bits(pkg, g, o, b):
    want, _ = oracle_wave(o, b)
    bits, nb = g.invalidate_bits(b)
    assert nb == len(want) and np.array_equal(pkg.fgi.bits_to_ids(bits), want)
    assert np.array_equal(g.last_wave_ids(), want)


def _after_async(pkg, g, o, b):
    want, _ = oracle_wave(o, b)
    t = g.invalidate_async_host(b)
    n_inv, ptr = g.wave_wait(t)
    assert n_inv == len(want) and ptr
    assert np.array_equal(g.wave_wait_ids(t), want)


def _after_batch(pkg, g, o, b):
    want, _ = oracle_wave(o, b)
    ids, _ = g.run_batch([("invalidate", b)])
    assert np.array_equal(np.sort(ids), want)


def _after_mutation(pkg, g, o, b):
    slots = np.asarray(b[:8], np.uint32)
    ver = np.arange(1 << 44, (1 << 44) + 2 * len(slots), 2, dtype=np.uint64) | np.uint64(1)
    o.clear_log()
    o.begin_compute_slots(slots, ver, None)
    g.begin_compute(slots, ver, None)
    assert np.array_equal(np.sort(g.last_wave_ids()), np.sort(o.inv_log()))
    o.clear_log()
    out_set, ids = g.set_output(slots)
    assert int(out_set.sum()) == o.set_output_slots(slots)
    assert np.array_equal(np.sort(ids), np.sort(o.inv_log()))
    want, _ = oracle_wave(o, b[8:])
    assert count_only(g, b[8:]) == len(want)
    assert np.array_equal(g.last_wave_ids(), want)


def _after_prune(pkg, g, o, b):
    ps = g.prune()
    _, ne = o.prune()
    assert ps.new_edges == ne
    want, _ = oracle_wave(o, b)
    assert count_only(g, b) == len(want)
    assert np.array_equal(g.last_wave_ids(), want)


@pytest.mark.parametrize("labels", [-1, 1])
@pytest.mark.parametrize("then", [_after_list, _after_bits, _after_async, _after_batch, _after_mutation, _after_prune],
                         ids=lambda f: f.__name__[7:])
def test_interleavings(pkg, gpu_available, then, labels):
    """A count-only wave A, then another driver from batch B, then a count-only wave C: states and ids are
    the oracle's after each."""
    scale = 12
    n = 1 << scale
    g, o, (a, b, c) = _rmat_pair(pkg, scale, labels, n_det=256)
    want_a, _ = oracle_wave(o, a)
    assert count_only(g, a) == len(want_a)
    then(pkg, g, o, b)
    assert_states_equal(g, o, n)
    want_c, _ = oracle_wave(o, c)
    assert count_only(g, c) == len(want_c)
    assert np.array_equal(g.last_wave_ids(), want_c)
    assert_states_equal(g, o, n)
    o.close()
    g.close()


# ---- flagged sets and views ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed_states():
    """The oracle's states over the 4,160 handles before the first wave of `_mixed` and after each wave."""
    arrays, waves, _ = _mixed()
    o = _oracle(MIXED_N, *arrays)
    states = [_dump_handles(o, MIXED_N, MIXED_DET, {})]
    for roots, imm, *_ in waves:
        o.invalidate_slots(roots, imm)
        states.append(_dump_handles(o, MIXED_N, MIXED_DET, {}))
    return states


@pytest.mark.parametrize("view_open", [False, True])
@pytest.mark.parametrize("labels", [-1, 1])
def test_flagged_sets_and_view(pkg, gpu_available, labels, view_open):
    """The 4,160-handle mixed-state graph: its waves flag nodes, so they keep their bitmap for the post-pass
    (and for the view's update) and start with the init kernel; the count-only calls give the same counts,
    flagged records and view planes as the list-returning ones, and the list on demand is right."""
    arrays, waves, o_end = _mixed()
    states = _mixed_states()
    g = _engine(pkg, MIXED_N, *arrays, labels=labels, n_detached=MIXED_DET)
    view = g.open_state_view() if view_open else None
    if view_open:
        assert_view(view, *states[0], "open")
    for k, (roots, imm, inv, ids, fl, _) in enumerate(waves):
        assert count_only(g, roots, imm) == len(inv), f"wave {k}"
        if view_open:
            assert_view(view, *states[k + 1], f"wave {k}")
        gi, gf = g.last_wave_flagged()
        assert np.array_equal(gi, ids) and np.array_equal(gf, fl), f"wave {k}"
        if k != 1:
            assert np.array_equal(g.last_wave_ids(), inv), f"wave {k}"
            gi, gf = g.last_wave_flagged()   # the list made on demand leaves the set readable
            assert np.array_equal(gi, ids) and np.array_equal(gf, fl), f"wave {k}"
    assert_states_equal(g, o_end, MIXED_N)
