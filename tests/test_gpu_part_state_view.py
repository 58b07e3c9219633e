"""The per-rank host-memory state view of a partition (fgi_part_state_view_open; C-ABI 0.7) against the CPU
oracle.

P ranks of an in-process group on one GPU (part_init_local: the RCCL path's own level loop; the accessor
runs no collective). A rank's planes address its local boundary handles: bit h < block is global slot
r * block + h in the host's numbering, the rank's detached handles follow. The expected planes of rank r are
the oracle's dump sliced to [r * block, min(N, (r + 1) * block)), zero-padded to block, then the rank's
detached handles, compared word for word (`assert_view` of test_gpu_state_view.py).

With labels = 1 the ranks' engines run on partition codes, so a wave reaches the planes through
k_view_part_wave; FGI_OPT_PART_VIEW_PATH pins its scatter and its gather form on these small graphs."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import fgo as O
from harness import COMPUTING, CONSISTENT, F_IOSO
from test_gpu_flagged import N, _dump_handles, _mixed, _oracle
from test_gpu_part_flagged import _build, _merged_step, _rank_records
from test_gpu_part_mutations import _check_states, _oracle_batch
from test_gpu_state_view import PLANES, _mixed_states, _mutation_plan, assert_view, planes_from_flags

gpu = pytest.mark.gpu

N_DET = 40
NONE = 0xFFFFFFFF
DIRECTIONS = {"auto": 0, "push": 1, "pull": 2}
# (labels, FGI_OPT_PART_VIEW_PATH): without codes k_view_wave runs as it is; with codes both forms pinned
CODES = [(0, 0), (1, 1), (1, 2)]


def _block(n, P):
    return -(-n // P)


def _rank_slice(v, f, r, block, n, n_det=N_DET):
    """Slots [r * block, min(n, (r + 1) * block)) of (v, f), zero-padded to block, then n_det empty handles."""
    lo, hi = r * block, min(n, (r + 1) * block)
    ev, ef = np.zeros(block + n_det, np.uint64), np.zeros(block + n_det, np.uint32)
    ev[:hi - lo], ef[:hi - lo] = v[lo:hi], f[lo:hi]
    return ev, ef


def _rank_states(o, r, block, n, det, n_det=N_DET):
    """The oracle's states over rank r's handles; det: the rank's detached handle -> oracle node."""
    v, f = _dump_handles(o, n, 0, {})
    ev, ef = _rank_slice(v, f, r, block, n, n_det)
    for gh, oh in det.items():
        _, ev[gh], ef[gh] = o.node_info(oh)
    return ev, ef


def _open(gs, block):
    views = []
    for r, g in enumerate(gs):
        view, base = g.part_open_state_view()
        assert base == r * block and view.n_handles == g.n_handles and view.words == (g.n_handles + 63) // 64
        views.append(view)
    return views


def _assert_routed(pkg, views, block, n, v, f, what):
    """fgi_part_view_is_consistent over every 97th global slot (and two past the end) against (v, f) over slots."""
    for s in list(range(0, n, 97)) + [n - 1]:
        want = bool(v[s] != 0 and (f[s] & 3) == CONSISTENT)
        assert pkg.fgi.part_view_is_consistent(views, block, s) == want, f"{what}: slot {s}"
    P = len(views)
    assert not pkg.fgi.part_view_is_consistent(views, block, P * block)
    assert not pkg.fgi.part_view_is_consistent(views, block, P * block + 1)


def _build_with(pkg, P, n, versions, flags, src, dst, tags, options, direction=0, labels=0, n_detached=N_DET):
    """`_build` of test_gpu_part_flagged.py with options set before anything is loaded (the first bulk load
    chooses the partition codes from the pull geometry of that moment)."""
    block = _block(n, P)
    gs = [pkg.Graph(block, n_detached=n_detached, rank=r, world=P, labels=labels) for r in range(P)]
    pkg.fgi.part_init_local(gs, n)
    present = np.nonzero(versions)[0].astype(np.uint32)
    for g in gs:
        g.set_option(pkg.fgi.OPT_DIRECTION, direction)
        for opt, value in options.items():
            g.set_option(opt, value)
        g.part_register_nodes(present, versions[present], flags[present])
        g.part_load_edges(src, dst, tags)
    return gs, block


def _pub(g):
    return g.view_stats().words_published


# ---- 1. the fixture is not vacuous (CPU only) ------------------------------------------------------------

@pytest.mark.parametrize("P", [2, 3, 8])
def test_fixture_is_not_vacuous(P):
    """Conditions on the oracle, not measurements: every rank's share of every wave's invalidated set holds at
    least 8 nodes (observed minimum 8), every wave invalidates at least 30 non-root nodes whose live invalidated
    parents all sit on other ranks (observed minimum 37), and wave 1 clears a delay_started bit."""
    (versions, _, src, dst, tags), waves, _ = _mixed()
    states = _mixed_states()
    block = _block(N, P)
    live = tags == versions[dst]
    for k, (roots, _, inv, *_rest) in enumerate(waves):
        share = np.bincount(inv // block, minlength=P)
        in_inv = np.zeros(N, bool)
        in_inv[inv] = True
        e = live & in_inv[src] & in_inv[dst]
        any_parent, local_parent, is_root = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, bool)
        any_parent[dst[e]] = True
        local_parent[dst[e & (src // block == dst // block)]] = True
        is_root[roots] = True
        cross = int(np.sum(any_parent & ~local_parent & ~is_root))
        print(f"P={P} wave {k}: shares {share.tolist()}, cross-rank-only {cross}")
        assert share.min() >= 8, (k, share)
        assert cross >= 30, (k, cross)
    a, b = planes_from_flags(*states[1]), planes_from_flags(*states[2])
    assert np.any(a["delay_started"] & ~b["delay_started"]), "wave 1 clears no delay_started bit"


# ---- 2. three mixed waves, read between ------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("labels,path", CODES)
@pytest.mark.parametrize("direction", list(DIRECTIONS))
@pytest.mark.parametrize("P", [2, 3, 8])
def test_three_waves_read_between(pkg, gpu_available, P, direction, labels, path):
    arrays, waves, o_end = _mixed()
    states = _mixed_states()
    # one pull tile per block, set before the load that chooses the codes: a rank's codes are dealt over the
    # runs of 1,024 slots of its range (two runs at P = 2 and 3; at P = 8 a rank's 512 slots are one run)
    gs, block = _build_with(pkg, P, N, *arrays, options={pkg.fgi.OPT_PULL_TPB: 1, pkg.fgi.OPT_PART_VIEW_PATH: path},
                            direction=DIRECTIONS[direction], labels=labels)
    if P == 3:
        assert block == 1366 and block % 64 != 0 and N - 2 * block < block   # a partial slot word, a short rank
    views = _open(gs, block)

    def check(k, what):
        v, f = states[k]
        for r, view in enumerate(views):
            assert_view(view, *_rank_slice(v, f, r, block, N), f"{what}, rank {r}")
        _assert_routed(pkg, views, block, N, v, f, what)

    check(0, "open")
    for k, (roots, imm, inv, ids, fl, _) in enumerate(waves):
        pkg.fgi.part_local_invalidate(gs, roots, imm)
        check(k + 1, f"wave {k}")   # straight after the call: nothing else has waited for the device yet
        got = np.concatenate([g.part_export_ids() for g in gs])
        assert np.array_equal(np.sort(got), inv), f"wave {k}: invalidated sets differ ({len(got)} vs {len(inv)})"
        recs = _rank_records(gs, N, block)
        gi, gf = _merged_step(recs, 0)
        assert np.array_equal(gi, ids) and np.array_equal(gf, fl), f"wave {k}: flagged {len(gi)} vs oracle {len(ids)}"
        check(k + 1, f"wave {k}, after the accessors")
    for g in gs:
        st = g.view_stats()
        print(f"P={P} {direction} labels={labels} path={path}: {st.as_dict()}")
        assert st.full_builds == 1 and st.updates >= 3
        assert st.extra_waits <= len(waves)   # at most one wait per cascade-running call
    # the engine's own report agrees once asked (it folds; the view must not have changed anything)
    _check_states(gs, o_end, N, block)
    check(3, "after dump_states")
    for g in gs:
        g.close()


# ---- 3. waits --------------------------------------------------------------------------------------------

@gpu
def test_a_rank_that_cannot_flag_waits_for_nothing_more(pkg, gpu_available):
    """An all-Consistent graph without delays (the flag gate is off): the host-driven wave, the planned one
    (the same wave again after fgi_restore) and one with the plan off each leave extra_waits at 0."""
    scale, seed, P = 12, 0x5EED0071, 2
    n = 1 << scale
    gs = [pkg.Graph(n // P, rank=r, world=P) for r in range(P)]
    pkg.fgi.part_init_local(gs, n)
    for g in gs:
        g.part_synth_rmat(scale, 8, seed, 0, 0)
    views = _open(gs, n // P)
    s, _ = O.gen_rmat(scale, 8, seed)
    roots = O.gen_roots(16, n, 0x5EED1071, np.bincount(s, minlength=n))
    for g in gs:
        g.snapshot()
    syncs = []
    for what in ("host-driven", "planned", "plan off"):
        if what == "plan off":
            for g in gs:
                g.set_option(pkg.fgi.OPT_PART_PLAN, 0)
        stats = pkg.fgi.part_local_invalidate(gs, roots)
        assert sum(x.v_inv for x in stats) > 16 and all(x.n_flagged == 0 for x in stats)
        syncs.append([x.host_syncs for x in stats])
        inv = np.sort(np.concatenate([g.part_export_ids() for g in gs]))
        for r, (g, view) in enumerate(zip(gs, views)):
            assert view.seq % 2 == 0
            got = np.flatnonzero(view.flags()[:n // P] == 2) + r * (n // P)
            assert np.array_equal(got, inv[inv // (n // P) == r]), f"{what}, rank {r}: Invalidated handles in the view"
            assert g.view_stats().extra_waits == 0, f"{what}, rank {r}"
        for g in gs:
            g.restore()
    print("host syncs per rank:", syncs)
    assert all(a < b for a, b in zip(syncs[1], syncs[0])), f"the second wave was not planned: {syncs}"
    for r, (g, view) in enumerate(zip(gs, views)):   # restored: every node Consistent again, as the engine reports
        _, f = g.dump_states()
        assert np.array_equal(view.flags(), f) and np.all(f[:n // P] == CONSISTENT)
        assert g.view_stats().extra_waits == 0
        g.close()


# ---- 4. dense and proportional ---------------------------------------------------------------------------

D_SCALE, D_EF, D_SEED = 14, 8, 0x5EED0072


@functools.lru_cache(maxsize=None)
def _dense_roots():
    n = 1 << D_SCALE
    s, _ = O.gen_rmat(D_SCALE, D_EF, D_SEED)
    deg = np.bincount(s, minlength=n)
    dense = O.gen_roots(64, n, 0x5EED1072, deg)
    leaves = np.flatnonzero(deg == 0)
    sparse = leaves[np.linspace(0, len(leaves) - 1, 16).astype(np.int64)].astype(np.uint32)   # over both ranks
    assert len(np.unique(sparse // 64)) == 16 and 4 <= int(np.sum(sparse < n // 2)) <= 12
    return dense, sparse


_single_dumps = {}


def _single(pkg):
    """The single-device engine's dumps after the sparse wave and after the dense one (computed once)."""
    if not _single_dumps:
        dense, sparse = _dense_roots()
        g = pkg.Graph(1 << D_SCALE)
        g.synth_rmat(D_SCALE, D_EF, D_SEED, 0, 0)
        assert np.array_equal(g.invalidate(sparse), sparse), "a root without dependants invalidates itself alone"
        _single_dumps["sparse"] = g.dump_states()
        n_inv = len(g.invalidate(dense))
        assert n_inv > (1 << D_SCALE) // 8, "not a dense wave"
        _single_dumps["dense"] = g.dump_states()
        g.close()
    return _single_dumps


@gpu
@pytest.mark.parametrize("labels,path", CODES + [(1, 0)])
def test_dense_and_proportional(pkg, gpu_available, labels, path):
    P, n = 2, 1 << D_SCALE
    block = n // P
    dense, sparse = _dense_roots()
    want = _single(pkg)
    gs = [pkg.Graph(block, rank=r, world=P, labels=labels) for r in range(P)]
    pkg.fgi.part_init_local(gs, n)
    for g in gs:
        g.part_synth_rmat(D_SCALE, D_EF, D_SEED, 0, 0)
        g.set_option(pkg.fgi.OPT_PART_VIEW_PATH, path)
    views = _open(gs, block)
    for what, roots in (("sparse", sparse), ("dense", dense)):
        before = [_pub(g) for g in gs]
        pkg.fgi.part_local_invalidate(gs, roots)
        v, f = want[what]
        for r, (g, view) in enumerate(zip(gs, views)):
            assert_view(view, *_rank_slice(v, f, r, block, n, 0), f"{what} wave, rank {r}")
            delta = _pub(g) - before[r]
            print(f"labels={labels} path={path} {what}: rank {r} published {delta} of {view.words} words per plane")
            # a wave moves the `consistent` plane only (no delays here): one word per 64 handles at most, and
            # a sparse wave no more words than it invalidates nodes
            assert 1 <= delta <= (16 if what == "sparse" else view.words), (what, r, delta)
    for g in gs:
        st = g.view_stats()
        assert st.full_builds == 1 and st.extra_waits == 0
        g.close()


# ---- 5. mutations and a batch ----------------------------------------------------------------------------

def _oracle_begin(o, dets, block, begin, newv, has_delay, out_detached):
    """begin_compute on the oracle; a displaced node that stays current lives on under its owner's detached handle."""
    old = [o.last(int(s)) for s in begin]
    o.begin_compute_slots(begin, newv, has_delay)
    for s, h_old, gh in zip(begin, old, out_detached):
        if gh != NONE:
            assert gh >= block
            dets[int(s) // block][int(gh)] = h_old


def _each_rank(gs, fn):
    """fn(rank, graph) on one host thread per rank: a collective call of an in-process group."""
    out, err = [None] * len(gs), []

    def run(r):
        try:
            out[r] = fn(r, gs[r])
        except Exception as e:   # noqa: BLE001 - reported below, on the test's thread
            err.append((r, e))
    ts = [threading.Thread(target=run, args=(r,)) for r in range(len(gs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not err, err
    return out


@gpu
@pytest.mark.parametrize("labels", [0, 1])
@pytest.mark.parametrize("P", [2, 3])
def test_mutations(pkg, gpu_available, P, labels):
    arrays, waves, _ = _mixed()
    begin, newv, has_delay, used_inv, used_ok = _mutation_plan()
    gs, block = _build(pkg, P, N, *arrays, labels=labels, n_detached=N_DET)
    o = _oracle(N, *arrays)
    dets = [{} for _ in range(P)]
    views = _open(gs, block)

    def check(what):
        for r, view in enumerate(views):
            assert_view(view, *_rank_states(o, r, block, N, dets[r]), f"{what}, rank {r}")

    # a wave first: the slot begin[0] is invalidated by its cascade and begun again below
    pkg.fgi.part_local_invalidate(gs, waves[0][0], waves[0][1])
    o.invalidate_slots(waves[0][0], waves[0][1])
    check("wave")
    # the direct calls (fgi_part_begin_compute / _add_used / _set_output), one host thread per rank: their own
    # view updates, not the batch's deferred one (test_batch)
    waits = [g.view_stats().extra_waits for g in gs]

    def waited(most, what):
        for r, g in enumerate(gs):
            now = g.view_stats().extra_waits
            assert now - waits[r] <= most, f"{what}, rank {r}: {now - waits[r]} further waits"
            waits[r] = now

    got = _each_rank(gs, lambda r, g: g.part_begin_compute(begin, newv, has_delay))
    out = np.array([got[int(s) // block][0][i] for i, s in enumerate(begin)], np.uint32)   # the owner's answer
    for r in range(P):
        others = np.array([int(s) // block != r for s in begin])
        assert np.all(got[r][0][others] == NONE), f"rank {r} reports a detached handle for a slot it does not own"
    _oracle_begin(o, dets, block, begin, newv, has_delay, out)
    assert sum(len(d) for d in dets) >= 2, "no detached handle appeared"
    check("begin_compute")
    waited(2, "begin_compute")   # its cascade's flagged records, then its own items
    # add_used: an already-Invalidated `used` gives the dependant InvalidateOnSetOutput
    deps, used = np.array([begin[1], begin[2]], np.uint32), np.array([used_inv, used_ok], np.uint32)
    got = _each_rank(gs, lambda r, g: g.part_add_used(deps, used))
    want = o.add_used_slots(deps, used)
    assert all(np.array_equal(res, want) for res in got) and want[0] == 2
    assert o.dump_states()[1][begin[1]] == COMPUTING | F_IOSO
    check("add_used")
    waited(1, "add_used")
    # set_output: begin[1] is invalidated at once (its cascade), the others become Consistent
    got = _each_rank(gs, lambda r, g: g.part_set_output(begin))
    o.set_output_slots(begin)
    assert all(list(out_set) == [1] * len(begin) for out_set, _ in got)
    assert int(begin[1]) in list(got[int(begin[1]) // block][1])
    check("set_output")
    waited(2, "set_output")
    # release one detached handle on its owner: no collective
    r_rel = next(r for r in range(P) if dets[r])
    rel = sorted(dets[r_rel])[0]
    gs[r_rel].release([rel])
    dets[r_rel].pop(rel)
    check("release")
    # invalidate_all: every rank's current nodes, one cascade
    got = _each_rank(gs, lambda r, g: g.part_invalidate_all())
    o.clear_log()
    o.invalidate_everything()
    assert np.array_equal(np.sort(np.concatenate(got)), np.sort(o.inv_log()))
    check("invalidate_all")
    for g in gs:
        assert g.view_stats().full_builds == 1
        g.close()
    o.close()


@gpu
@pytest.mark.parametrize("labels", [0, 1])
@pytest.mark.parametrize("P", [2, 3])
def test_batch(pkg, gpu_available, P, labels):
    arrays, waves, _ = _mixed()
    begin, newv, has_delay, used_inv, used_ok = _mutation_plan()
    gs, block = _build(pkg, P, N, *arrays, labels=labels, n_detached=N_DET)
    o = _oracle(N, *arrays)
    dets = [{} for _ in range(P)]
    views = _open(gs, block)
    deps, used = np.array([begin[1], begin[2]], np.uint32), np.array([used_inv, used_ok], np.uint32)
    steps = [("invalidate", waves[0][0], waves[0][1]), ("begin_compute", begin, newv, has_delay),
             ("add_used", deps, used), ("set_output", begin[1:]), ("invalidate", waves[1][0], waves[1][1])]
    ids, outs, _ = pkg.fgi.part_local_run_batch(gs, steps)
    old = [o.last(int(s)) for s in begin]   # step 0 replaces no node: the nodes step 1 displaces
    want, oouts = _oracle_batch(o, steps)
    assert np.array_equal(np.sort(ids), np.sort(want)) and np.array_equal(outs[2], oouts[2])
    for s, h_old, gh in zip(begin, old, outs[1]):
        if gh != NONE:
            assert gh >= block
            dets[int(s) // block][int(gh)] = h_old
    assert sum(len(d) for d in dets) >= 2, "no detached handle appeared"
    assert (o.dump_states()[1][begin[0]] & 3) == COMPUTING   # invalidated in cascade 0, begun again, never set
    for r, view in enumerate(views):
        assert_view(view, *_rank_states(o, r, block, N, dets[r]), f"run_batch, rank {r}")
    for g in gs:
        assert g.view_stats().full_builds == 1
        g.close()
    o.close()


# ---- 6. open late, close, restore ------------------------------------------------------------------------

@gpu
def test_open_late_close_restore(pkg, gpu_available):
    arrays, waves, _ = _mixed()
    states = _mixed_states()
    P = 2
    gs, block = _build(pkg, P, N, *arrays, labels=1, n_detached=N_DET)
    never = gs[0].view_stats()
    assert (never.updates, never.words_published, never.full_builds, never.extra_waits) == (0, 0, 0, 0)
    for k in range(2):
        pkg.fgi.part_local_invalidate(gs, waves[k][0], waves[k][1])   # visits unfolded at open
    for g in gs:
        st = g.view_stats()   # a partition that never opened a view
        assert (st.updates, st.words_published, st.full_builds, st.extra_waits) == (0, 0, 0, 0)
    views = _open(gs, block)

    def check(k, what):
        for r, view in enumerate(views):
            assert_view(view, *_rank_slice(*states[k], r, block, N), f"{what}, rank {r}")

    check(2, "open after two waves")
    for g in gs:
        g.snapshot()
    at_snapshot = [{k: getattr(v, k).copy() for k in PLANES} for v in views]
    pkg.fgi.part_local_invalidate(gs, waves[2][0], waves[2][1])
    check(3, "the third wave")
    assert any(np.any(getattr(views[r], k) != at_snapshot[r][k]) for r in range(P) for k in PLANES)
    for g in gs:
        g.restore()
    for r in range(P):
        for k in PLANES:
            assert np.array_equal(getattr(views[r], k), at_snapshot[r][k]), f"rank {r}: plane {k} after restore"
    check(2, "restore")
    for g in gs:
        g.close_state_view()
    pkg.fgi.part_local_invalidate(gs, waves[2][0], waves[2][1])
    check(2, "a closed view is no longer updated")
    builds = [g.view_stats().full_builds for g in gs]
    again = _open(gs, block)
    for r in range(P):
        assert again[r].struct.consistent == views[r].struct.consistent and again[r].struct.seq == views[r].struct.seq
        assert gs[r].view_stats().full_builds == builds[r] + 1
    check(3, "reopened")
    for g in gs:
        g.close()
    # opened on an empty partition: the registration is one full build, the move of the installed words when
    # the first bulk load chooses the codes is another, and a synthetic graph is one, codes chosen or not
    block = _block(N, P)
    gs = [pkg.Graph(block, n_detached=N_DET, rank=r, world=P, labels=1) for r in range(P)]
    pkg.fgi.part_init_local(gs, N)
    views = _open(gs, block)
    empty = (np.zeros(N, np.uint64), np.zeros(N, np.uint32))
    for r, view in enumerate(views):
        assert_view(view, *_rank_slice(*empty, r, block, N), f"empty, rank {r}")
    versions, flags, src, dst, tags = arrays
    present = np.nonzero(versions)[0].astype(np.uint32)
    for g in gs:
        g.part_register_nodes(present, versions[present], flags[present])
    check(0, "registered")
    for g in gs:
        g.part_load_edges(src, dst, tags)
    check(0, "codes chosen with the words installed")
    assert [g.view_stats().full_builds for g in gs] == [3] * P
    pkg.fgi.part_local_invalidate(gs, waves[0][0], waves[0][1])
    check(1, "a wave on the codes")
    for g in gs:
        g.close()
    scale, seed = 10, 0x5EED0073
    m = 1 << scale
    rs = [pkg.Graph(m // P, rank=r, world=P, labels=1) for r in range(P)]
    pkg.fgi.part_init_local(rs, m)
    sviews = _open(rs, m // P)
    for g in rs:
        g.part_synth_rmat(scale, 8, seed, 0, 0)
    for r, (g, view) in enumerate(zip(rs, sviews)):
        v, f = g.dump_states()
        assert np.all(f == CONSISTENT) and np.array_equal(view.flags(), f) and view.seq % 2 == 0
        assert g.view_stats().full_builds == 2, f"rank {r}: open, then one build for the synthetic graph"
        g.close()
    single = pkg.Graph(64)
    sv = pkg.fgi.StateViewStruct()
    sv.struct_size = C.sizeof(sv)
    assert single.lib.fgi_part_state_view_open(single.h, C.byref(sv), None) == pkg.fgi.ENOTSUP
    with pytest.raises(pkg.FgiError) as e:
        single.part_open_state_view()
    assert e.value.status == pkg.fgi.ENOTSUP
    single.close()
