"""fgi_part_last_flagged: the nodes a partitioned cascade only flagged, rank by rank, against the CPU oracle.

P ranks of an in-process group on one GPU (LocalComm: the RCCL path's own level loop, only the collectives are
device copies). The accessor runs no collective, so what a rank reports here is what it reports on its own GPU.
The expected sets are differences of two oracle dumps (`expected_flagged` of test_gpu_flagged.py), split by
owner: block = ceil(N / P). The engine's states are never read between the waves of a multi-wave case (a dump
folds the visit bitmap into the node words)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fgo as O
from harness import COMPUTING, CONSISTENT, F_DS, F_HD, F_IOSO
from test_gpu_flagged import N, _mixed, expected_flagged
from test_gpu_part_mutations import _check_states, _group

U32P = C.POINTER(C.c_uint32)
gpu = pytest.mark.gpu


def _block(n, P):
    return -(-n // P)


def _build(pkg, P, n, versions, flags, src, dst, tags, direction=0, labels=0, n_detached=64):
    block = _block(n, P)
    gs = [pkg.Graph(block, n_detached=n_detached, rank=r, world=P, labels=labels) for r in range(P)]
    pkg.fgi.part_init_local(gs, n)
    present = np.nonzero(versions)[0].astype(np.uint32)
    for g in gs:
        g.set_option(pkg.fgi.OPT_DIRECTION, direction)
        g.part_register_nodes(present, versions[present], flags[present])
        if len(src):
            g.part_load_edges(src, dst, tags)
    return gs, block


def _rank_records(gs, n, block, n_steps=1):
    """Every rank's (steps, ids, flags), checked for step order, ascending ids within a step and ownership."""
    recs = []
    for r, g in enumerate(gs):
        steps, ids, flags = g.part_last_flagged()
        assert len(steps) == len(ids) == len(flags)
        assert np.all(np.diff(steps.astype(np.int64)) >= 0), f"rank {r}: records not in step order"
        assert len(steps) == 0 or int(steps[-1]) < n_steps, f"rank {r}: step {steps[-1]} of {n_steps}"
        for k in np.unique(steps):
            assert np.all(np.diff(ids[steps == k].astype(np.int64)) > 0), f"rank {r}, step {k}: ids not ascending"
        lo, hi = r * block, min(n, (r + 1) * block)
        assert np.all((ids >= lo) & (ids < hi)), f"rank {r}: a record outside [{lo}, {hi}): {ids}"
        recs.append((steps, ids, flags))
    return recs


def _merged_step(recs, k):
    """Step k's records of all ranks in rank order: the ranks own ascending ranges, so ascending ids."""
    ids = np.concatenate([i[s == k] for s, i, _ in recs]).astype(np.uint32)
    flags = np.concatenate([f[s == k] for s, _, f in recs]).astype(np.uint32)
    return ids, flags


def _wave(pkg, gs, n, block, roots, imm, inv, ids, fl, what):
    stats = pkg.fgi.part_local_invalidate(gs, roots, imm)
    got = np.concatenate([g.part_export_ids() for g in gs])
    assert np.array_equal(np.sort(got), inv), f"{what}: invalidated sets differ ({len(got)} vs {len(inv)})"
    recs = _rank_records(gs, n, block)
    assert all(np.all(s == 0) for s, _, _ in recs), f"{what}: a single cascade reports step 0"
    gi, gf = _merged_step(recs, 0)
    assert np.array_equal(gi, ids), f"{what}: flagged {len(gi)} vs oracle {len(ids)}"
    assert np.array_equal(gf, fl), f"{what}: flags differ"
    return stats, recs


# ---- 1. the fixture is not vacuous (CPU only) ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _shares(P):
    """Per wave of _mixed(): the ranks' shares of the flagged set, and how many flagged nodes have live
    invalidated parents (edge tag == the dependant's version) on other ranks only."""
    (versions, _, src, dst, tags), waves, _ = _mixed()
    block = _block(N, P)
    live = tags == versions[dst]
    out = []
    for _, _, inv, ids, _, _ in waves:
        in_inv = np.zeros(N, bool)
        in_inv[inv] = True
        e = live & in_inv[src]
        flagged = np.zeros(N, bool)
        flagged[ids] = True
        e &= flagged[dst]
        any_parent = np.zeros(N, bool)
        any_parent[dst[e]] = True
        same = e & (src // block == dst // block)
        local_parent = np.zeros(N, bool)
        local_parent[dst[same]] = True
        cross_only = int(np.sum(any_parent & ~local_parent))
        out.append((np.bincount(ids // block, minlength=P).tolist(), cross_only))
    return out


@pytest.mark.parametrize("P", [2, 3, 8])
def test_fixture_is_not_vacuous(P):
    """Every rank has something to report and every wave flags nodes that only a visit from another rank can
    have reached; a changed generator must not let the partition cases pass on nothing."""
    sh = _shares(P)
    assert [sum(s) for s, _ in sh] == [73, 29, 36]
    for k, (share, cross) in enumerate(sh):
        print(f"P={P} wave {k + 1}: shares {share}, cross-rank-only {cross}")
        if P == 8:
            assert sum(1 for c in share if c) >= 7, (k, share)
        else:
            assert all(c > 0 for c in share), (k, share)
        assert cross >= 10, (k, cross)


# ---- 2. three mixed-state waves --------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("labels", [0, 1])
@pytest.mark.parametrize("direction", [0, 1, 2])
@pytest.mark.parametrize("P", [2, 3, 8])
def test_three_mixed_waves(pkg, gpu_available, P, direction, labels):
    arrays, waves, o_end = _mixed()
    gs, block = _build(pkg, P, N, *arrays, direction=direction, labels=labels)
    for k, (roots, imm, inv, ids, fl, _) in enumerate(waves):
        _wave(pkg, gs, N, block, roots, imm, inv, ids, fl, f"wave {k}")
    _check_states(gs, o_end, N, block)
    for g in gs:
        g.close()


# ---- 3. planned waves and small buckets ------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("P", [2, 4])
def test_planned_waves_and_small_buckets(pkg, gpu_available, P):
    """The same wave host-driven, planned (one wait: the post-pass adds none) and planned with buckets of one
    id per peer, whose wave repeats its final collect: the post-pass runs behind the last one only."""
    arrays, waves, _ = _mixed()
    gs, block = _build(pkg, P, N, *arrays, direction=0)
    for g in gs:
        g.snapshot()
    roots, imm, inv, ids, fl, _ = waves[0]
    _wave(pkg, gs, N, block, roots, imm, inv, ids, fl, "host-driven")
    for g in gs:
        g.restore()
    stats, _ = _wave(pkg, gs, N, block, roots, imm, inv, ids, fl, "planned")
    assert all(x.host_syncs == 2 for x in stats), [x.host_syncs for x in stats]
    for g in gs:
        g.set_option(pkg.fgi.OPT_PART_BUCKET, 2)
        g.restore()
    _wave(pkg, gs, N, block, roots, imm, inv, ids, fl, "planned, small buckets")
    for g in gs:
        g.close()


# ---- 4. a hand-sized cross-rank case ---------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("direction", [0, 1, 2])
def test_hand_sized_cross_rank(pkg, gpu_available, direction):
    n, P = 64, 2
    versions = O.version_of(3, np.arange(n, dtype=np.uint64)).copy()
    flags = np.full(n, CONSISTENT, np.uint32)
    flags[[6, 32]] |= F_HD
    flags[40] = COMPUTING
    src = np.array([5, 5, 31, 31, 32], np.uint32)
    dst = np.array([6, 31, 32, 40, 33], np.uint32)
    tags = versions[dst]
    o = O.Oracle(n)
    o.load_graph(versions, flags, src, dst, tags)
    gs, block = _build(pkg, P, n, versions, flags, src, dst, tags, direction=direction, n_detached=0)
    assert block == 32
    want = [([5], None, [5, 31], [6, 32, 40], [CONSISTENT | F_DS | F_HD, CONSISTENT | F_DS | F_HD, COMPUTING | F_IOSO]),
            ([32, 40], [1, 1], [32, 33], [40], [COMPUTING | F_IOSO | F_DS])]
    for k, (roots, imm, w_inv, w_ids, w_fl) in enumerate(want):
        before = o.dump_states()
        o.clear_log()
        o.invalidate_slots(roots, imm)
        inv = np.sort(o.inv_log())
        ids, fl = expected_flagged(before, o.dump_states())
        # the values read from the code; the oracle decides
        assert list(inv) == w_inv and list(ids) == w_ids and list(fl) == w_fl, (k, inv, ids, fl)
        if k == 0:
            assert o.dump_states()[1][33] == CONSISTENT   # behind the delayed 32: wave A does not reach it
        _, recs = _wave(pkg, gs, n, block, np.array(roots, np.uint32), None if imm is None else np.array(imm, np.uint8),
                        inv, ids, fl, f"wave {'AB'[k]}")
        for r in range(P):
            own = (ids // block) == r
            assert np.array_equal(recs[r][1], ids[own]) and np.array_equal(recs[r][2], fl[own]), (k, r, recs[r])
    _check_states(gs, o, n, block)
    o.close()


# ---- 5. batches ------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("P", [2, 3])
def test_batch_cascades(pkg, gpu_available, P):
    """test_displacement_and_set_output_cascades' graph with every slot multiplied by 8: its edges cross ranks."""
    n = 96
    versions = O.version_of(5, np.arange(n, dtype=np.uint64)).copy()
    flags = np.full(n, CONSISTENT, np.uint32)
    flags[[8, 32, 48, 64]] = COMPUTING
    flags[[16, 40, 56]] |= F_HD
    src = np.array([0, 0, 0, 24, 24, 24, 8], np.uint32)
    dst = np.array([8, 16, 64, 40, 48, 32, 56], np.uint32)
    tags = versions[dst]
    gs, block = _group(pkg, P, n)
    slots = np.arange(n, dtype=np.uint32)
    for g in gs:
        g.part_register_nodes(slots, versions, flags)
        g.part_load_edges(src, dst, tags)
    o = O.Oracle(n)
    o.load_graph(versions, flags, src, dst, tags)
    bc = np.array([24, 32], np.uint32)
    newv = (versions[bc] + np.uint64(1000)).astype(np.uint64)
    steps = [("invalidate", [0]), ("begin_compute", bc, newv, np.zeros(2, np.uint8)), ("set_output", [8]),
             ("invalidate", [64], [1])]
    exp = []
    o.clear_log()
    for sp in steps:
        before = o.dump_states()
        if sp[0] == "invalidate":
            o.invalidate_slots(sp[1], sp[2] if len(sp) > 2 else None)
        elif sp[0] == "begin_compute":
            o.begin_compute_slots(sp[1], sp[2], sp[3])
        else:
            assert o.set_output_slots(sp[1]) == 1
        exp.append(expected_flagged(before, o.dump_states()))
    assert [list(e[0]) for e in exp] == [[8, 16, 64], [40, 48], [56], [64]]
    ids, outs, _ = pkg.fgi.part_local_run_batch(gs, steps)
    assert np.array_equal(np.sort(ids), np.sort(o.inv_log()))
    recs = _rank_records(gs, n, block, len(steps))   # every record sits on its owner
    per = [_merged_step(recs, k) for k in range(len(steps))]
    for k in range(len(steps)):
        assert np.array_equal(per[k][0], exp[k][0]), f"step {k}: {per[k][0]} vs {exp[k][0]}"
        assert np.array_equal(per[k][1], exp[k][1]), f"step {k}: flags {per[k][1]} vs {exp[k][1]}"
    # 64 under steps 0 and 3, with different flags
    assert per[0][1][list(per[0][0]).index(64)] == COMPUTING | F_IOSO
    assert list(per[3][0]) == [64] and list(per[3][1]) == [COMPUTING | F_IOSO | F_DS]
    # the Computing own slot is not reported under step 1
    assert 32 not in per[1][0]
    _check_states(gs, o, n, block)
    o.close()


# ---- 6. streaming rounds whose timers come from the engine -----------------------------------------------

@gpu
@pytest.mark.parametrize("P", [2, 3])
def test_stream_mix_timers_from_the_ranks(pkg, gpu_available, P):
    """test_stream_mix_timers_from_the_engine's loop over fgi_part_local_run_batch: round r + 1's timers are
    the union over the ranks of the last step's records that carry DelayStarted, not the closed form."""
    from test_gpu_stream import _mix, _oracle_round
    mix = _mix(pkg, 40, 30, 4, 10, 0x5EED00E0)
    n = mix.n
    used, dep, tag = mix.initial_edges()
    flags = mix.state_flags()
    gs, block = _group(pkg, P, n)
    slots = np.arange(n, dtype=np.uint32)
    for g in gs:
        g.part_register_nodes(slots, mix.version, flags)
        g.part_load_edges(used, dep, tag)
    o = O.Oracle(n)
    o.load_graph(mix.version.copy(), flags, used, dep, tag)
    prev = np.zeros(0, np.uint32)
    timers = np.zeros(0, np.uint32)
    for r in range(8):
        _, hs, ls = mix.plan(prev)
        vh = mix.new_versions(hs).copy()
        vl = mix.new_versions(ls).copy()
        t_oracle = _oracle_round(o, mix, timers, hs, ls, vh, vl)
        roots = mix.roots(r)
        before = o.dump_states()
        o.clear_log()
        o.invalidate_slots(roots)
        w_oracle = o.inv_log()
        exp, expf = expected_flagged(before, o.dump_states())
        steps = []
        if len(timers):
            steps.append(("invalidate", timers, np.ones(len(timers), np.uint8)))
        steps += [("begin_compute", hs, vh), ("set_output", hs), ("begin_compute", ls, vl, mix.has_delay[ls]),
                  ("add_used", ls, mix.hub_of(ls)), ("set_output", ls), ("invalidate", roots)]
        ids, _, _ = pkg.fgi.part_local_run_batch(gs, steps)
        want = np.concatenate([t_oracle, w_oracle]).astype(np.uint32)
        assert np.array_equal(np.sort(ids), np.sort(want)), f"round {r}: invalidated ids differ as a multiset"
        gi, gf = _merged_step(_rank_records(gs, n, block, len(steps)), len(steps) - 1)
        assert len(gi) >= 1, f"round {r}: nothing reported"
        assert np.array_equal(gi, exp) and np.array_equal(gf, expf), f"round {r}: {len(gi)} vs oracle {len(exp)}"
        timers = gi[(gf & F_DS) != 0]
        assert np.array_equal(timers, np.sort(mix.plan(roots)[0])), f"round {r}: timers differ from the closed form"
        prev = roots
    _check_states(gs, o, n, block)
    o.close()


# ---- 7. world size 1 over RCCL ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("collectives", [1, 0])
def test_rccl_world1(pkg, gpu_available, collectives):
    """fgi_part_init's path (the one a multi-GPU node runs) at world size 1, with and without its collectives."""
    import torch
    from harness import random_states
    scale, ef, seed = 11, 8, 3
    n = 1 << scale
    rng = np.random.default_rng(77)
    versions, flags = random_states(n, rng, seed=seed)
    s, d = O.gen_rmat(scale, ef, seed)
    live = (versions[s] != 0) & ((flags[s] & 3) == CONSISTENT)
    s, d = s[live], d[live]
    tags = versions[d].astype(np.uint64).copy()
    tags[tags == 0] = 7
    tags[rng.random(len(s)) < 0.2] += np.uint64(1)
    g = pkg.Graph(n, n_detached=64, rank=0, world=1)
    g.part_init(n, pkg.fgi.part_unique_id())
    g.set_option(pkg.fgi.OPT_PART_COLLECTIVES, collectives)
    present = np.nonzero(versions)[0].astype(np.uint32)
    g.part_register_nodes(present, versions[present], flags[present])
    g.part_load_edges(s, d, tags)
    o = O.Oracle(n)
    o.load_graph(versions, flags, s, d, tags)
    total = 0
    for wave in range(2):
        roots = rng.integers(0, n, 48).astype(np.uint32)
        imm = (rng.random(48) < 0.3).astype(np.uint8)
        before = o.dump_states()
        o.clear_log()
        o.invalidate_slots(roots, imm)
        exp, expf = expected_flagged(before, o.dump_states())
        d_roots = torch.from_numpy(roots.astype(np.int32)).cuda()
        d_imm = torch.from_numpy(imm).cuda()
        n_inv = g.part_invalidate(len(roots), d_roots.data_ptr(), d_imm.data_ptr())
        ids = g.part_export_ids()
        assert n_inv == len(ids) and np.array_equal(np.sort(ids), np.sort(o.inv_log())), wave
        steps, gi, gf = g.part_last_flagged()
        assert np.all(steps == 0) and np.all(np.diff(gi.astype(np.int64)) > 0)
        assert np.array_equal(gi, exp), f"wave {wave}: flagged {len(gi)} vs oracle {len(exp)}"
        assert np.array_equal(gf, expf), f"wave {wave}: flags differ"
        total += len(exp)
    assert total >= 10, total
    v, f = g.dump_states()
    ov, of = o.dump_states()
    assert np.array_equal(v[:n], ov) and np.array_equal(f[:n], of)
    o.close()
    g.close()


# ---- 8. contract -----------------------------------------------------------------------------------------

@gpu
def test_accessor_contract(pkg, gpu_available):
    fgi = pkg.fgi
    n = C.c_uint64(7)
    single = pkg.Graph(64)
    assert single.lib.fgi_part_last_flagged(single.h, None, None, None, 0, C.byref(n)) == fgi.ENOTSUP
    single.close()
    arrays, waves, _ = _mixed()
    P = 2
    gs, block = _build(pkg, P, N, *arrays)
    for g in gs:   # before any wave
        assert all(len(a) == 0 for a in g.part_last_flagged())
        g.snapshot()
    roots, imm, inv, ids, fl, _ = waves[0]
    _wave(pkg, gs, N, block, roots, imm, inv, ids, fl, "wave 1")
    g = gs[0]
    own = ids < block
    need = int(own.sum())
    assert need >= 2
    st_, gi, gf = (np.zeros(need, np.uint32) for _ in range(3))

    def p(a):
        return a.ctypes.data_as(U32P)

    n.value = 0
    assert g.lib.fgi_part_last_flagged(g.h, None, None, None, 0, C.byref(n)) == fgi.OK and n.value == need
    n.value = 0
    assert g.lib.fgi_part_last_flagged(g.h, p(st_), p(gi), p(gf), need - 1, C.byref(n)) == fgi.ECAPACITY
    assert n.value == need
    assert g.lib.fgi_part_last_flagged(g.h, None, p(gi), None, need, C.byref(n)) == fgi.OK
    assert np.array_equal(gi, ids[own])
    assert g.lib.fgi_part_last_flagged(g.h, p(st_), p(gi), p(gf), need, C.byref(n)) == fgi.OK
    assert np.all(st_ == 0) and np.array_equal(gi, ids[own]) and np.array_equal(gf, fl[own])
    # the single-device accessors do not report a partition
    for call in (g.last_wave_flagged, g.last_batch_flagged):
        with pytest.raises(pkg.FgiError) as e:
            call()
        assert e.value.status == fgi.ENOTSUP
    # a later partitioned wave replaces the records
    roots, imm, inv, ids2, fl2, _ = waves[1]
    _wave(pkg, gs, N, block, roots, imm, inv, ids2, fl2, "wave 2")
    # after fgi_restore: no records
    for g in gs:
        g.restore()
        assert all(len(a) == 0 for a in g.part_last_flagged())
    # and the restored graph reports wave 1 again
    roots, imm, inv, ids, fl, _ = waves[0]
    _wave(pkg, gs, N, block, roots, imm, inv, ids, fl, "wave 1 again")
    for g in gs:
        g.close()
    # a partition that cannot flag: empty sets, no flagged visits
    scale, seed = 10, 0x5EED0024
    m = 1 << scale
    rs = [pkg.Graph(m // P, rank=r, world=P) for r in range(P)]
    fgi.part_init_local(rs, m)
    for r in rs:
        r.part_synth_rmat(scale, 8, seed, 0, 0)
    s, _ = O.gen_rmat(scale, 8, seed)
    roots = O.gen_roots(16, m, 0x5EED1024, np.bincount(s, minlength=m))
    stats = fgi.part_local_invalidate(rs, roots)
    assert sum(x.v_inv for x in stats) > 16 and all(x.n_flagged == 0 for x in stats)
    for r in rs:
        assert all(len(a) == 0 for a in r.part_last_flagged())
        r.close()
