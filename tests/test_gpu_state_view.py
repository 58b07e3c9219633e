"""The host-memory state view (fgi_state_view_open; C-ABI 0.6) against the CPU oracle.

The view is six bit planes in host memory that the device keeps current: a node's state is read with a
load, without an engine call. Every case turns the oracle's dump into planes (`planes_from_flags`) and
compares them word for word with the engine's, and `view.flags()` with the oracle's `dump_states()`.
Unlike `dump_states` / `get_state`, reading the view does not fold the visit bitmap into the node words,
so the three-wave case reads the engine's states between its waves and still checks every wave's
flagged set (tests/test_gpu_flagged.py cannot).

Handles: 4,096 slots + 40 detached, so the last plane word is partial (4,136 = 64 * 64 + 40)."""
import functools

import numpy as np
import pytest

import fgo as O
from harness import COMPUTING, CONSISTENT, F_DS, F_HD, F_IOSO, INVALIDATED
from test_gpu_flagged import DIRECTIONS, _dump_handles, _engine, _mixed, _oracle

gpu = pytest.mark.gpu

N = 4096
N_DET = 40
PLANES = ("registered", "consistent", "computing", "ioso", "delay_started", "has_delay")
NONE = 0xFFFFFFFF


def _pack(bits):
    """A boolean per handle -> 64-bit words, bit h % 64 of word h // 64."""
    n = len(bits)
    padded = np.zeros((n + 63) // 64 * 64, np.uint8)
    padded[:n] = bits
    return np.packbits(padded, bitorder="little").view(np.uint64)


def planes_from_flags(versions, flags):
    """The six planes of fgi_state_view for canonical (version, state_flags) arrays over the handles."""
    versions, flags = np.asarray(versions, np.uint64), np.asarray(flags, np.uint32)
    reg = versions != 0
    st = flags & 3
    return {
        "registered": _pack(reg),
        "consistent": _pack(reg & (st == CONSISTENT)),
        "computing": _pack(reg & (st == COMPUTING)),
        "ioso": _pack(reg & ((flags & F_IOSO) != 0)),
        "delay_started": _pack(reg & ((flags & F_DS) != 0)),
        "has_delay": _pack(reg & ((flags & F_HD) != 0)),
    }


def flags_from_planes(planes, n):
    """fgi_view_flags over every handle, restated on numpy (the decode the C helper does per handle)."""
    b = {k: np.unpackbits(planes[k].view(np.uint8), bitorder="little")[:n].astype(np.uint32) for k in PLANES}
    f = np.where(b["consistent"] == 1, CONSISTENT | (b["delay_started"] * F_DS),
                 np.where(b["computing"] == 1, COMPUTING | (b["ioso"] * F_IOSO) | (b["delay_started"] * F_DS), INVALIDATED))
    return ((f | (b["has_delay"] * F_HD)) * b["registered"]).astype(np.uint32)


def assert_view(view, versions, flags, what):
    exp = planes_from_flags(versions, flags)
    for name in PLANES:
        got = getattr(view, name)
        bad = np.nonzero(got != exp[name])[0]
        assert len(bad) == 0, f"{what}: plane {name} differs at words {bad[:8]}: {got[bad[:8]]} vs {exp[name][bad[:8]]}"
    want = np.where(np.asarray(versions) != 0, flags, 0).astype(np.uint32)
    assert np.array_equal(view.flags(), want), f"{what}: view.flags() differs from the oracle's dump"
    assert view.seq % 2 == 0, f"{what}: seq is odd after a synchronous call"


def _handles(o, det=None):
    return _dump_handles(o, N, N_DET, det or {})


@functools.lru_cache(maxsize=None)
def _mixed_states():
    """The oracle's states over the handles before the first wave of `_mixed` and after each wave."""
    arrays, waves, _ = _mixed()
    o = _oracle(N, *arrays)
    states = [_handles(o)]
    for roots, imm, *_ in waves:
        o.invalidate_slots(roots, imm)
        states.append(_handles(o))
    return states


def test_oracle_waves_move_every_plane_a_wave_can_move():
    """CPU only: keeps the three-wave case from passing on nothing. Every wave changes at least one bit in
    each of `consistent`, `ioso` and `delay_started`, and at least one wave clears a `delay_started` bit (a
    delayed Consistent node that had started its delay and that an `immediately` root invalidates)."""
    _, waves, _ = _mixed()
    assert [len(w[3]) for w in waves] == [73, 29, 36]
    states = _mixed_states()
    cleared = 0
    for k in range(3):
        a, b = planes_from_flags(*states[k]), planes_from_flags(*states[k + 1])
        for name in ("consistent", "ioso", "delay_started"):
            assert np.any(a[name] != b[name]), f"wave {k} leaves plane {name} unchanged"
        cleared += int(np.sum([bin(int(x)).count("1") for x in a["delay_started"] & ~b["delay_started"]]))
    assert cleared >= 1, "no wave clears a delay_started bit"


@gpu
@pytest.mark.parametrize("labels", [-1, 1])
@pytest.mark.parametrize("direction", list(DIRECTIONS))
def test_three_waves_read_between(pkg, gpu_available, direction, labels):
    arrays, waves, _ = _mixed()
    states = _mixed_states()
    g = _engine(pkg, N, *arrays, labels=labels, n_detached=N_DET, direction=DIRECTIONS[direction])
    view = g.open_state_view()
    assert view.n_handles == N + N_DET and view.words == (N + N_DET + 63) // 64
    assert_view(view, *states[0], "open")
    for k, (roots, imm, inv, ids, fl, _) in enumerate(waves):
        got = g.invalidate(roots, imm)
        assert np.array_equal(got, inv), f"wave {k}: invalidated sets differ"
        assert_view(view, *states[k + 1], f"wave {k}")
        gi, gf = g.last_wave_flagged()
        assert np.array_equal(gi, ids), f"wave {k}: flagged {len(gi)} vs oracle {len(ids)}"
        assert np.array_equal(gf, fl), f"wave {k}: flags differ"
        assert all(view.is_consistent(int(h)) == bool((states[k + 1][1][h] & 3) == CONSISTENT and states[k + 1][0][h])
                   for h in range(0, N + N_DET, 97))
    st = g.view_stats()
    assert st.full_builds == 1 and st.updates >= 3
    # the engine's own report agrees once asked (it folds; the view must not have changed anything)
    gv, gf = g.dump_states()
    assert np.array_equal(gf, np.where(states[3][0] != 0, states[3][1], 0))
    assert_view(view, *states[3], "after dump_states")


@gpu
@pytest.mark.parametrize("labels", [-1, 1])
def test_open_on_a_populated_graph(pkg, gpu_available, labels):
    arrays, waves, _ = _mixed()
    states = _mixed_states()
    g = _engine(pkg, N, *arrays, labels=labels, n_detached=N_DET)
    g.invalidate(waves[0][0], waves[0][1])   # visits unfolded at open
    view = g.open_state_view()
    assert_view(view, *states[1], "open after a wave")
    assert g.view_stats().full_builds == 1
    again = g.open_state_view()   # the same planes
    assert again.struct.consistent == view.struct.consistent and g.view_stats().full_builds == 1
    g.invalidate(waves[1][0], waves[1][1])
    assert_view(view, *states[2], "the wave after")
    g.close_state_view()
    g.invalidate(waves[2][0], waves[2][1])
    assert_view(view, *states[2], "a closed view is no longer updated")
    view = g.open_state_view()
    assert_view(view, *states[3], "reopened")
    assert g.view_stats().full_builds == 2


# ---- dense waves and proportional cost: R-MAT scale 16 ----------------------------------------------
SCALE, EF, SEED, STALE, STALE_SEED = 16, 16, 0x5EED0061, 50, 0x5EED0062


@functools.lru_cache(maxsize=None)
def _rmat():
    n = 1 << SCALE
    s, d = O.gen_rmat(SCALE, EF, SEED)
    versions = O.version_of(SEED, np.arange(n, dtype=np.uint64))
    tags = O.gen_tags(s, d, SEED, STALE, STALE_SEED)
    deg = np.bincount(s, minlength=n)
    roots = O.gen_roots(256, n, 0x5EED1061, deg)
    return n, versions, s, d, tags, deg, roots


@functools.lru_cache(maxsize=None)
def _rmat_expected(entry):
    n, versions, s, d, tags, deg, roots = _rmat()
    o = O.Oracle(n)
    o.load_graph(versions, None, s, d, tags)
    if entry == "invalidate_all":
        o.invalidate_everything()
    elif entry == "leaf":
        o.invalidate_slots(np.array([_leaf()], np.uint32))
    else:
        o.invalidate_slots(roots)
    out = o.dump_states(), np.sort(o.inv_log())
    o.close()
    return out


def _leaf():
    """A slot without dependants: its wave invalidates it alone."""
    deg = _rmat()[5]
    return int(np.nonzero(deg == 0)[0][0])


def _rmat_graph(pkg, labels):
    g = pkg.Graph(1 << SCALE, labels=labels)
    g.synth_rmat(SCALE, EF, SEED, STALE, STALE_SEED)
    return g


@gpu
@pytest.mark.parametrize("labels", [-1, 1])
@pytest.mark.parametrize("entry", ["invalidate", "invalidate_bits", "invalidate_all"])
def test_dense_wave(pkg, gpu_available, entry, labels):
    n, versions, *_, roots = _rmat()
    (ov, of), inv = _rmat_expected("invalidate_all" if entry == "invalidate_all" else "invalidate")
    g = _rmat_graph(pkg, labels)
    view = g.open_state_view()
    assert_view(view, versions, np.full(n, CONSISTENT, np.uint32), "open")
    if entry == "invalidate":
        assert np.array_equal(g.invalidate(roots), inv)
    elif entry == "invalidate_bits":
        bits, n_inv = g.invalidate_bits(roots)
        assert n_inv == len(inv) and np.array_equal(pkg.fgi.bits_to_ids(bits), inv)
    else:
        assert np.array_equal(g.invalidate_all(), inv)
    assert len(inv) > n // 8, "not a dense wave"
    assert_view(view, ov, of, entry)
    st = g.view_stats()
    assert st.full_builds == 1 and st.extra_waits == 0   # a graph that cannot flag pays no further wait


@gpu
@pytest.mark.parametrize("labels", [-1, 1])
def test_cost_is_proportional(pkg, gpu_available, labels):
    n, versions, *_ = _rmat()
    (ov, of), inv = _rmat_expected("leaf")
    assert list(inv) == [_leaf()]
    g = _rmat_graph(pkg, labels)
    view = g.open_state_view()
    before = g.view_stats()
    assert np.array_equal(g.invalidate([_leaf()]), inv)
    after = g.view_stats()
    assert_view(view, ov, of, "leaf wave")
    assert after.full_builds == before.full_builds
    assert 1 <= after.words_published - before.words_published <= 8


# ---- mutations and a batch --------------------------------------------------------------------------
def _pick(flags, versions, pred, k, taken):
    out = [int(h) for h in np.nonzero(pred & (versions != 0))[0] if int(h) not in taken][:k]
    assert len(out) == k
    taken.update(out)
    return out


def _mutation_plan():
    """Slots of the mixed graph for the mutation steps: Consistent, delayed and Invalidated slots to begin
    again, an Invalidated `used` for add_used, and one slot that wave 0 invalidates."""
    (versions, flags, *_), waves, _ = _mixed()
    st = flags & 3
    taken = set()
    hit = [int(h) for h in waves[0][2] if (flags[h] & F_HD) == 0][:1]   # invalidated by step 0's cascade
    taken.update(hit)
    cons = _pick(flags, versions, (st == CONSISTENT) & ((flags & F_HD) == 0), 2, taken)
    delayed = _pick(flags, versions, (st == CONSISTENT) & ((flags & F_HD) != 0), 2, taken)
    inval = _pick(flags, versions, st == INVALIDATED, 1, taken)
    used_inv = _pick(flags, versions, st == INVALIDATED, 1, taken)
    used_ok = _pick(flags, versions, (st == CONSISTENT) & ((flags & F_HD) == 0), 1, taken)
    begin = np.array(hit + cons + delayed + inval, np.uint32)
    newv = (versions[begin] + np.uint64(1000)).astype(np.uint64)
    has_delay = np.zeros(len(begin), np.uint8)
    has_delay[2] = 1
    return begin, newv, has_delay, used_inv[0], used_ok[0]


def _oracle_begin(o, det, begin, newv, has_delay, out_detached):
    old = [o.last(int(s)) for s in begin]
    o.begin_compute_slots(begin, newv, has_delay)
    for s, h_old, gh in zip(begin, old, out_detached):
        if gh != NONE:
            assert gh >= N
            det[int(gh)] = h_old


@gpu
@pytest.mark.parametrize("labels", [-1, 1])
def test_mutations(pkg, gpu_available, labels):
    arrays, waves, _ = _mixed()
    begin, newv, has_delay, used_inv, used_ok = _mutation_plan()
    g = _engine(pkg, N, *arrays, labels=labels, n_detached=N_DET)
    o = _oracle(N, *arrays)
    det = {}
    view = g.open_state_view()
    # a wave first: the slot `begin[0]` is invalidated by its cascade and begun again below
    g.invalidate(waves[0][0], waves[0][1])
    o.invalidate_slots(waves[0][0], waves[0][1])
    assert_view(view, *_handles(o, det), "wave")
    out = g.begin_compute(begin, newv, has_delay)
    _oracle_begin(o, det, begin, newv, has_delay, out)
    assert len(det) >= 2, "no detached handle appeared"
    assert_view(view, *_handles(o, det), "begin_compute")
    # add_used: an already-Invalidated `used` gives the dependant InvalidateOnSetOutput
    deps, used = np.array([begin[1], begin[2]], np.uint32), np.array([used_inv, used_ok], np.uint32)
    res = g.add_used(deps, used)
    assert np.array_equal(res, o.add_used_slots(deps, used)) and res[0] == 2
    v, f = _handles(o, det)
    assert f[begin[1]] == COMPUTING | F_IOSO
    assert_view(view, v, f, "add_used")
    # set_output: begin[1] is invalidated at once (its cascade), the others become Consistent
    out_set, ids = g.set_output(begin)
    o.set_output_slots(begin)
    assert list(out_set) == [1] * len(begin) and int(begin[1]) in list(ids)
    assert_view(view, *_handles(o, det), "set_output")
    rel = sorted(det)[0]
    g.release([rel])
    det.pop(rel)
    assert_view(view, *_handles(o, det), "release")
    assert g.view_stats().full_builds == 1


@gpu
@pytest.mark.parametrize("labels", [-1, 1])
def test_batch(pkg, gpu_available, labels):
    arrays, waves, _ = _mixed()
    begin, newv, has_delay, used_inv, used_ok = _mutation_plan()
    g = _engine(pkg, N, *arrays, labels=labels, n_detached=N_DET)
    o = _oracle(N, *arrays)
    det = {}
    view = g.open_state_view()
    deps, used = np.array([begin[1], begin[2]], np.uint32), np.array([used_inv, used_ok], np.uint32)
    ids, outs = g.run_batch([("invalidate", waves[0][0], waves[0][1]), ("begin_compute", begin, newv, has_delay),
                             ("add_used", deps, used), ("set_output", begin[1:]),
                             ("invalidate", waves[1][0], waves[1][1])])
    o.invalidate_slots(waves[0][0], waves[0][1])
    assert int(begin[0]) in list(np.sort(o.inv_log())), "step 0's cascade does not reach the slot begun again"
    _oracle_begin(o, det, begin, newv, has_delay, outs[1])
    o.add_used_slots(deps, used)
    o.set_output_slots(begin[1:])
    o.invalidate_slots(waves[1][0], waves[1][1])
    v, f = _handles(o, det)
    assert (f[begin[0]] & 3) == COMPUTING   # invalidated in cascade 1, begun again in step 2, never set
    assert_view(view, v, f, "run_batch")
    assert g.view_stats().full_builds == 1


@gpu
@pytest.mark.parametrize("labels", [-1, 1])
def test_async_pair(pkg, gpu_available, labels):
    arrays, waves, _ = _mixed()
    states = _mixed_states()
    g = _engine(pkg, N, *arrays, labels=labels, n_detached=N_DET)
    view = g.open_state_view()
    t1 = g.invalidate_async_host(waves[0][0], waves[0][1])
    t2 = g.invalidate_async_host(waves[1][0], waves[1][1])
    assert view.seq % 2 == 1, "seq must be odd while waves are in flight"
    assert np.array_equal(g.wave_wait_ids(t2), waves[1][2])
    assert_view(view, *states[2], "after waiting for the second ticket")
    assert np.array_equal(g.wave_wait_ids(t1), waves[0][2])
    gi, gf = g.wave_wait_flagged(t2)
    assert np.array_equal(gi, waves[1][3]) and np.array_equal(gf, waves[1][4])


@gpu
@pytest.mark.parametrize("mutate", [False, True])
def test_snapshot_restore(pkg, gpu_available, mutate):
    arrays, waves, _ = _mixed()
    states = _mixed_states()
    begin, newv, has_delay, *_ = _mutation_plan()
    g = _engine(pkg, N, *arrays, n_detached=N_DET)
    view = g.open_state_view()
    g.invalidate(waves[0][0], waves[0][1])
    g.snapshot()
    at_snapshot = {k: getattr(view, k).copy() for k in PLANES}
    assert_view(view, *states[1], "snapshot")
    g.invalidate(waves[1][0], waves[1][1])
    if mutate:   # the node words are copied back
        g.begin_compute(begin, newv, has_delay)
    assert any(np.any(getattr(view, k) != at_snapshot[k]) for k in PLANES)
    g.restore()
    for k in PLANES:
        assert np.array_equal(getattr(view, k), at_snapshot[k]), f"plane {k} after restore"
    assert_view(view, *states[1], "restore")
    g.invalidate(waves[1][0], waves[1][1])
    assert_view(view, *states[2], "the wave after restore")


@gpu
def test_never_opened_and_partitioned(pkg, gpu_available):
    arrays, waves, _ = _mixed()
    g = _engine(pkg, N, *arrays, n_detached=N_DET)
    g.invalidate(waves[0][0], waves[0][1])
    st = g.view_stats()
    assert (st.updates, st.words_published, st.full_builds, st.extra_waits) == (0, 0, 0, 0)
    gs = [pkg.Graph(512, rank=r, world=2) for r in range(2)]
    pkg.fgi.part_init_local(gs, 1024)
    with pytest.raises(pkg.FgiError) as e:
        gs[0].open_state_view()
    assert e.value.status == pkg.fgi.ENOTSUP
