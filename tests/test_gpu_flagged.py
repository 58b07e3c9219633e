"""The flagged set of a call (fgi_last_wave_flagged / fgi_wave_wait_flagged) against the CPU oracle.

Computed.Invalidate() has two branches that do not invalidate (Computed.cs:173-178: a Computing node only
gets InvalidateOnSetOutput, plus InvalidationDelayStarted from an `immediately` root; Computed.cs:186-197: a
Consistent node with an InvalidationDelay only gets InvalidationDelayStarted). The engine lists the nodes a
call flagged that way. The expected set is a difference of two oracle dumps (`expected_flagged`): which
visit sets a flag first depends on the order, the set does not.

The engine's states are never read between the waves of a multi-wave case (dump_states / get_state fold
the visit bitmap into the node words, which would hide a node being reported by two consecutive waves)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fgo as O
from harness import (COMPUTING, CONSISTENT, F_DS, F_HD, F_IOSO, INVALIDATED, assert_states_equal, random_states)

pytestmark = pytest.mark.gpu

N = 4096
N_DET = 64
DIRECTIONS = {"push": 1, "pull": 2, "auto": 0}


def expected_flagged(before, after):
    """Handles whose canonical flags gained IOSO / DelayStarted, not invalidated, same node (version)."""
    (bv, bf), (av, af) = before, after
    gained = (af & (F_IOSO | F_DS) & ~bf) != 0
    keep = gained & ((af & 3) != INVALIDATED) & (av == bv)
    ids = np.nonzero(keep)[0].astype(np.uint32)
    return ids, af[ids]


def _edges_from_live(versions, flags, rng, m, n, stale_p=0.3):
    # as test_gpu_parity.py: only Consistent nodes have `_usedBy` entries
    live = np.nonzero((versions != 0) & ((flags & 3) == CONSISTENT))[0].astype(np.uint32)
    src = rng.choice(live, m).astype(np.uint32)
    dst = rng.integers(0, n, m).astype(np.uint32)
    tags = versions[dst].astype(np.uint64).copy()
    tags[tags == 0] = 7
    stale = rng.random(m) < stale_p
    tags[stale] += np.uint64(1)
    return src, dst, tags


def _oracle(n, versions, flags, src, dst, tags):
    o = O.Oracle(n)
    o.load_graph(versions, flags, src, dst, tags)
    return o


def _engine(pkg, n, versions, flags, src, dst, tags, labels=-1, n_detached=N_DET, direction=None):
    g = pkg.Graph(n, n_detached=n_detached, labels=labels)
    if direction is not None:
        g.set_option(pkg.fgi.OPT_DIRECTION, direction)
    present = np.nonzero(versions)[0].astype(np.uint32)
    g.register_nodes(present, versions[present], flags[present])
    if len(src):
        g.load_edges(src, dst, tags)
    return g


@functools.lru_cache(maxsize=None)
def _mixed():
    """Case 1's graph and its three waves on the oracle (computed once, read-only afterwards): the graph
    arrays, per wave (roots, imm, invalidated ids, flagged ids, their flags), and the oracle after wave 3."""
    rng = np.random.default_rng(7)
    versions, flags = random_states(N, rng)
    src, dst, tags = _edges_from_live(versions, flags, rng, 6000, N)
    o = _oracle(N, versions, flags, src, dst, tags)
    waves = []
    for _ in range(3):
        roots = rng.integers(0, N, 48).astype(np.uint32)
        imm = (rng.random(48) < 0.3).astype(np.uint8)
        before = o.dump_states()
        o.clear_log()
        o.invalidate_slots(roots, imm)
        ids, fl = expected_flagged(before, o.dump_states())
        waves.append((roots, imm, np.sort(o.inv_log()), ids, fl, before[1][ids]))
    return (versions, flags, src, dst, tags), waves, o


def test_oracle_waves_are_not_vacuous():
    """A changed generator must not let the cases pass on nothing: the oracle alone gives 73 / 29 / 36
    flagged nodes, every wave has at least 20 with both kinds among them, and wave 2 holds a Computing node
    that already had InvalidateOnSetOutput and gains only DelayStarted from an `immediately` root (with
    this draw order wave 3 holds none: 0 / 1 / 0 such nodes)."""
    _, waves, _ = _mixed()
    assert [len(w[3]) for w in waves] == [73, 29, 36]
    ioso_to_ds = []
    for _, _, _, ids, fl, bf in waves:
        assert len(ids) >= 20
        assert np.any((fl & 3) == COMPUTING) and np.any(((fl & 3) == CONSISTENT) & ((fl & F_DS) != 0))
        ioso_to_ds.append(int(np.sum(((fl & 3) == COMPUTING) & ((bf & F_IOSO) != 0) & ((fl & F_DS) != 0))))
    assert ioso_to_ds[1] >= 1, ioso_to_ds


@pytest.mark.parametrize("labels", [-1, 1])
@pytest.mark.parametrize("direction", list(DIRECTIONS))
def test_random_mixed_states_three_waves(pkg, gpu_available, direction, labels):
    arrays, waves, o_end = _mixed()
    g = _engine(pkg, N, *arrays, labels=labels, direction=DIRECTIONS[direction])
    for k, (roots, imm, inv, ids, fl, _) in enumerate(waves):
        got = g.invalidate(roots, imm)
        assert np.array_equal(got, inv), f"wave {k}: invalidated sets differ"
        gi, gf = g.last_wave_flagged()
        assert np.all(np.diff(gi.astype(np.int64)) > 0), f"wave {k}: ids not ascending"
        assert np.array_equal(gi, ids), f"wave {k}: flagged {len(gi)} vs oracle {len(ids)}"
        assert np.array_equal(gf, fl), f"wave {k}: flags differ"
    assert_states_equal(g, o_end, N)


def _chain():
    n = 6
    versions = O.version_of(3, np.arange(n, dtype=np.uint64)).copy()
    flags = np.full(n, CONSISTENT, np.uint32)
    flags[3] |= F_HD
    src = np.array([0, 1, 2, 3], np.uint32)
    dst = np.array([1, 2, 3, 4], np.uint32)
    return n, versions, flags, src, dst


def test_chain(pkg, gpu_available):
    n, versions, flags, src, dst = _chain()
    g = _engine(pkg, n, versions, flags, src, dst, versions[dst], n_detached=0)
    assert list(g.invalidate([0])) == [0, 1, 2]
    ids, fl = g.last_wave_flagged()
    assert list(ids) == [3] and list(fl) == [CONSISTENT | F_DS | F_HD]
    assert list(g.invalidate([0])) == []
    assert list(g.last_wave_flagged()[0]) == []
    assert list(g.invalidate([3], [1])) == [3, 4]
    assert list(g.last_wave_flagged()[0]) == []
    # a Computing leaf hanging off node 1 in a fresh graph
    flags2 = flags.copy()
    flags2[5] = COMPUTING
    src2, dst2 = np.append(src, 1).astype(np.uint32), np.append(dst, 5).astype(np.uint32)
    g2 = _engine(pkg, n, versions, flags2, src2, dst2, versions[dst2], n_detached=0)
    assert list(g2.invalidate([1])) == [1, 2]
    ids, fl = g2.last_wave_flagged()
    assert list(ids) == [3, 5] and list(fl) == [CONSISTENT | F_DS | F_HD, COMPUTING | F_IOSO]
    g3 = _engine(pkg, n, versions, flags2, src2[4:], dst2[4:], versions[dst2[4:]], n_detached=0)
    assert list(g3.invalidate([1])) == [1]
    ids, fl = g3.last_wave_flagged()
    assert list(ids) == [5] and list(fl) == [COMPUTING | F_IOSO]


def test_flagged_and_invalidated_in_one_wave(pkg, gpu_available):
    """Node 3 (delayed) is reached by the cascade from 0 and is an `immediately` root of the same wave."""
    n, versions, flags, src, dst = _chain()
    g = _engine(pkg, n, versions, flags, src, dst, versions[dst], n_detached=0)
    o = _oracle(n, versions, flags, src, dst, versions[dst])
    before = o.dump_states()
    o.invalidate_slots([0, 3], [0, 1])
    exp, _ = expected_flagged(before, o.dump_states())
    assert list(exp) == []
    assert list(g.invalidate([0, 3], [0, 1])) == [0, 1, 2, 3, 4]
    assert list(g.last_wave_flagged()[0]) == []
    # the next wave does not report it either
    g.invalidate([0])
    assert list(g.last_wave_flagged()[0]) == []
    assert_states_equal(g, o, n)


def test_invalidate_bits_then_flagged(pkg, gpu_available):
    arrays, waves, _ = _mixed()
    g = _engine(pkg, N, *arrays)
    for roots, imm, inv, ids, fl, _ in waves[:2]:
        bits, n_inv = g.invalidate_bits(roots, imm)
        assert n_inv == len(inv)
        gi, gf = g.last_wave_flagged()
        assert np.array_equal(gi, ids) and np.array_equal(gf, fl)
        assert np.array_equal(g.last_wave_ids(), inv)   # the list made on demand leaves the set readable
        gi, gf = g.last_wave_flagged()
        assert np.array_equal(gi, ids) and np.array_equal(gf, fl)


@pytest.mark.parametrize("labels", [-1, 1])
def test_async_pair(pkg, gpu_available, labels):
    arrays, waves, _ = _mixed()
    g = _engine(pkg, N, *arrays, labels=labels)
    t1 = g.invalidate_async_host(waves[0][0], waves[0][1])
    t2 = g.invalidate_async_host(waves[1][0], waves[1][1])
    for t, w in ((t1, waves[0]), (t2, waves[1]), (t1, waves[0])):   # t1 again: the same list
        gi, gf = g.wave_wait_flagged(t)
        assert np.array_equal(gi, w[3]), f"ticket {t}: flagged {len(gi)} vs oracle {len(w[3])}"
        assert np.array_equal(gf, w[4])
    assert np.array_equal(g.wave_wait_ids(t1), waves[0][2]) and np.array_equal(g.wave_wait_ids(t2), waves[1][2])
    # the last call's set is the last ticket's
    gi, gf = g.last_wave_flagged()
    assert np.array_equal(gi, waves[1][3]) and np.array_equal(gf, waves[1][4])


def _dump_handles(o, n, n_det, det):
    """The oracle's states over the engine's handles: slots, then detached handle -> oracle node."""
    v, f = o.dump_states()
    v, f = np.append(v, np.zeros(n_det, np.uint64)), np.append(f, np.zeros(n_det, np.uint32))
    for gh, oh in det.items():
        _, v[gh], f[gh] = o.node_info(oh)
    return v, f


def test_cascade_entry_points(pkg, gpu_available):
    """begin_compute's displacement cascade, a detached root, set_output's cascade — each against the
    oracle's dump difference over the engine's handles."""
    n, n_det = 8, 4
    versions = O.version_of(5, np.arange(n, dtype=np.uint64)).copy()
    flags = np.full(n, CONSISTENT, np.uint32)
    flags[1] |= F_HD                  # B: delayed dependant of A (slot 0)
    flags[2] = COMPUTING | F_IOSO     # C: its set_output cascades to the delayed D (slot 3)
    flags[3] |= F_HD
    flags[4] = COMPUTING              # E: displaced while Computing -> detached
    flags[5] |= F_HD                  # F: displaced while delayed -> detached, DelayStarted
    src, dst = np.array([0, 2, 5], np.uint32), np.array([1, 3, 6], np.uint32)
    tags = versions[dst]
    g = _engine(pkg, n, versions, flags, src, dst, tags, n_detached=n_det)
    o = _oracle(n, versions, flags, src, dst, tags)
    det = {}
    # 1. begin_compute displaces A (invalidated; B flagged), E and F (flagged, but their slots hold new nodes)
    slots = np.array([0, 4, 5], np.uint32)
    newv = versions[slots] + np.uint64(1000)
    before = _dump_handles(o, n, n_det, det)
    dh = g.begin_compute(slots, newv, np.zeros(3, np.uint8))
    for s, v, h in zip(slots, newv, dh):
        _, displaced = o.begin_compute(int(s), int(v), False)
        if h != 0xFFFFFFFF:
            det[int(h)] = displaced
    assert dh[0] == 0xFFFFFFFF and dh[1] >= n and dh[2] >= n
    exp, expf = expected_flagged(before, _dump_handles(o, n, n_det, det))
    assert list(exp) == [1]
    gi, gf = g.last_wave_flagged()
    assert np.array_equal(gi, exp) and np.array_equal(gf, expf)
    assert list(g.last_wave_ids()) == [0]
    # the detached F carries its DelayStarted (the host starts its timer from out_detached)
    assert g.get_state([int(dh[2])])[1][0] == CONSISTENT | F_DS | F_HD
    # 2. roots: the detached E with `immediately` (gains DelayStarted) and B again (nothing new)
    before = _dump_handles(o, n, n_det, det)
    o.invalidate_nodes([det[int(dh[1])]], [1])
    o.invalidate_slots([1])
    exp, expf = expected_flagged(before, _dump_handles(o, n, n_det, det))
    assert list(exp) == [int(dh[1])] and list(expf) == [COMPUTING | F_IOSO | F_DS]
    g.invalidate(np.array([dh[1], 1], np.uint32), np.array([1, 0], np.uint8))
    gi, gf = g.last_wave_flagged()
    assert np.array_equal(gi, exp) and np.array_equal(gf, expf)
    # 3. set_output on the IOSO node C: invalidated at once, the cascade flags D
    before = _dump_handles(o, n, n_det, det)
    o.set_output(o.last(2))
    exp, expf = expected_flagged(before, _dump_handles(o, n, n_det, det))
    assert list(exp) == [3]
    out_set, ids = g.set_output([2])
    assert list(out_set) == [1] and list(ids) == [2]
    gi, gf = g.last_wave_flagged()
    assert np.array_equal(gi, exp) and np.array_equal(gf, expf)
    # 4. a set_output without a cascade reports nothing
    g.set_output([0])
    o.set_output(o.last(0))
    assert list(g.last_wave_flagged()[0]) == []
    assert_states_equal(g, o, n)


@pytest.mark.parametrize("labels", [-1, 1])
def test_invalidate_all(pkg, gpu_available, labels):
    arrays, _, _ = _mixed()
    g = _engine(pkg, N, *arrays, labels=labels)
    o = _oracle(N, *arrays)
    before = o.dump_states()
    o.clear_log()
    o.invalidate_everything()
    exp, expf = expected_flagged(before, o.dump_states())
    assert len(exp) > 300
    ids = g.invalidate_all()
    assert np.array_equal(ids, np.sort(o.inv_log()))
    gi, gf = g.last_wave_flagged()
    assert np.array_equal(gi, exp) and np.array_equal(gf, expf)
    assert_states_equal(g, o, N)


def test_capacity_gate_and_batches(pkg, gpu_available):
    arrays, waves, _ = _mixed()
    g = _engine(pkg, N, *arrays)
    g.invalidate(waves[0][0], waves[0][1])
    need = len(waves[0][3])
    ids, fl, n = np.zeros(need, np.uint32), np.zeros(need, np.uint32), C.c_uint64()
    u32p = C.POINTER(C.c_uint32)
    st = g.lib.fgi_last_wave_flagged(g.h, ids.ctypes.data_as(u32p), fl.ctypes.data_as(u32p), need - 1, C.byref(n))
    assert st == pkg.fgi.ECAPACITY and n.value == need
    st = g.lib.fgi_last_wave_flagged(g.h, ids.ctypes.data_as(u32p), None, need, C.byref(n))   # flags are optional
    assert st == pkg.fgi.OK and np.array_equal(ids, waves[0][3])
    # after a batch the set is not reported
    g.run_batch([("invalidate", waves[1][0])])
    with pytest.raises(pkg.FgiError) as e:
        g.last_wave_flagged()
    assert e.value.status == pkg.fgi.ENOTSUP and "fgi_run_batch" in str(e.value)
    # a single wave reports again, and only what it flagged itself
    o = _oracle(N, *arrays)
    o.invalidate_slots(waves[0][0], waves[0][1])
    o.invalidate_slots(waves[1][0])
    before = o.dump_states()
    o.invalidate_slots(waves[2][0], waves[2][1])
    exp, expf = expected_flagged(before, o.dump_states())
    g.invalidate(waves[2][0], waves[2][1])
    gi, gf = g.last_wave_flagged()
    assert np.array_equal(gi, exp) and np.array_equal(gf, expf)
    # gate: an all-Consistent graph without delays cannot flag anything
    scale, seed = 10, 0x5EED0024
    r = pkg.Graph(1 << scale)
    r.synth_rmat(scale, 8, seed, 0, 0)
    s, _ = O.gen_rmat(scale, 8, seed)
    roots = O.gen_roots(16, 1 << scale, 0x5EED1024, np.bincount(s, minlength=1 << scale))
    assert len(r.invalidate(roots)) > 16
    gi, gf = r.last_wave_flagged()
    assert len(gi) == 0 and len(gf) == 0
