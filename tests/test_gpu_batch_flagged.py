"""fgi_last_batch_flagged: the nodes each cascade of a batch only flagged, against the CPU oracle.

A batch's cascades (k_wave_coop) fold their visits into the node words themselves; a handle whose fold changes
its word without invalidating it is recorded there, and an `immediately` root on a Computing node records
itself. The expected sets are differences of two oracle dumps around each step (`expected_flagged` of
test_gpu_flagged.py: gained bits, not Invalidated, same version, which also drops a begin_compute step's own
slots). The engine's states are never read between the batches of a multi-batch case."""
import ctypes as C

import numpy as np
import pytest

import fgo as O
from harness import COMPUTING, CONSISTENT, F_DS, F_HD, F_IOSO, assert_states_equal, build_pair
from test_gpu_flagged import N, _dump_handles, _engine, _mixed, _oracle, expected_flagged
from test_gpu_part_mutations import _group
from test_gpu_stream import _mix, _oracle_round

pytestmark = pytest.mark.gpu

U32P = C.POINTER(C.c_uint32)


def _by_step(rec, n_steps):
    """(steps, ids, flags) -> per step (ids, flags); the records come in step order."""
    steps, ids, flags = rec
    assert len(steps) == len(ids) == len(flags)
    assert np.all(np.diff(steps.astype(np.int64)) >= 0), "records not in step order"
    assert len(steps) == 0 or int(steps[-1]) < n_steps
    return [(ids[steps == k], flags[steps == k]) for k in range(n_steps)]


def _assert_step(got, ids, flags, what):
    gi, gf = got
    assert np.all(np.diff(gi.astype(np.int64)) > 0), f"{what}: ids not ascending"
    assert np.array_equal(gi, ids), f"{what}: flagged {len(gi)} vs oracle {len(ids)}"
    assert np.array_equal(gf, flags), f"{what}: flags differ"


@pytest.mark.parametrize("labels", [-1, 1])
def test_three_waves_as_one_batch(pkg, gpu_available, labels):
    arrays, waves, o_end = _mixed()
    g = _engine(pkg, N, *arrays, labels=labels)
    ids, _ = g.run_batch([("invalidate", w[0], w[1]) for w in waves])
    assert np.array_equal(ids, np.concatenate([w[2] for w in waves]).astype(np.uint32))
    per = _by_step(g.last_batch_flagged(), 3)
    for k, w in enumerate(waves):
        _assert_step(per[k], w[3], w[4], f"step {k}")
    # a handle under two steps (a Computing node flagged by one wave gains DelayStarted from a later
    # `immediately` root): whether this draw has one is the oracle's word
    want_twice = np.array([h for h in np.unique(np.concatenate([w[3] for w in waves]))
                           if sum(h in w[3] for w in waves) > 1], np.uint32)
    all_ids = np.concatenate([p[0] for p in per])
    u, c = np.unique(all_ids, return_counts=True)
    assert np.array_equal(u[c > 1], want_twice)
    assert_states_equal(g, o_end, N)


def test_three_waves_as_three_batches(pkg, gpu_available):
    arrays, waves, o_end = _mixed()
    g = _engine(pkg, N, *arrays)
    for k, w in enumerate(waves):
        ids, _ = g.run_batch([("invalidate", w[0], w[1])])
        assert np.array_equal(ids, w[2]), f"batch {k}"
        _assert_step(_by_step(g.last_batch_flagged(), 1)[0], w[3], w[4], f"batch {k}")
    assert_states_equal(g, o_end, N)


@pytest.mark.parametrize("hubs,leaves,k,delay_pct", [(40, 30, 4, 10), (64, 200, 8, 5), (7, 1, 7, 50)])
def test_stream_mix_timers_from_the_engine(pkg, gpu_available, hubs, leaves, k, delay_pct):
    """test_gpu_batch.py's streaming rounds, but round r + 1's timers are what the engine reported for round
    r's hub wave (the last step's records that carry DelayStarted), not the workload's closed form."""
    mix = _mix(pkg, hubs, leaves, k, delay_pct, 0x5EED00E0)
    n = mix.n
    used, dep, tag = mix.initial_edges()
    g, o = build_pair(pkg, n, mix.version.copy(), mix.state_flags(), used, dep, tag)
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
        st = pkg.fgi.BatchStats()
        ids, _ = g.run_batch(steps, stats=st)
        assert st.host_syncs <= 2, st.as_dict()
        want = np.concatenate([np.sort(t_oracle), np.sort(w_oracle)]).astype(np.uint32)
        assert np.array_equal(ids, want), f"round {r}"
        gi, gf = _by_step(g.last_batch_flagged(), len(steps))[-1]
        assert len(gi) >= 1, f"round {r}: nothing reported"
        _assert_step((gi, gf), exp, expf, f"round {r}")
        timers = gi[(gf & F_DS) != 0]
        assert np.array_equal(timers, np.sort(mix.plan(roots)[0])), f"round {r}: timers differ from the closed form"
        prev = roots
    assert_states_equal(g, o, n)
    g.close()
    o.close()


def test_displacement_and_set_output_cascades(pkg, gpu_available):
    n, n_det = 12, 4
    versions = O.version_of(5, np.arange(n, dtype=np.uint64)).copy()
    flags = np.full(n, CONSISTENT, np.uint32)
    flags[[1, 4, 6, 8]] = COMPUTING        # 1, 8: reached by step 0; 6: by step 1; 4: displaced while Computing
    flags[[2, 5, 7]] |= F_HD               # delayed dependants of 0 (step 0), 3 (step 1), 1 (step 2)
    src = np.array([0, 0, 0, 3, 3, 3, 1], np.uint32)
    dst = np.array([1, 2, 8, 5, 6, 4, 7], np.uint32)
    tags = versions[dst]
    g = _engine(pkg, n, versions, flags, src, dst, tags, n_detached=n_det)
    o = _oracle(n, versions, flags, src, dst, tags)
    slots = np.array([3, 4], np.uint32)
    newv = (versions[slots] + np.uint64(1000)).astype(np.uint64)
    ids, outs = g.run_batch([("invalidate", [0]), ("begin_compute", slots, newv, np.zeros(2, np.uint8)),
                             ("set_output", [1]), ("invalidate", [8], [1])])
    dh = outs[1]
    assert dh[0] == pkg.fgi.NONE and dh[1] >= n
    per = _by_step(g.last_batch_flagged(), 4)
    # the oracle, call by call; detached engine handle -> oracle node once step 1 has made it
    det, exp = {}, []
    o.clear_log()
    before = _dump_handles(o, n, n_det, det)
    o.invalidate_slots([0])
    exp.append(expected_flagged(before, _dump_handles(o, n, n_det, det)))
    before = _dump_handles(o, n, n_det, det)
    for s, v, h in zip(slots, newv, dh):
        _, displaced = o.begin_compute(int(s), int(v), False)
        if h != pkg.fgi.NONE:
            det[int(h)] = displaced
    exp.append(expected_flagged(before, _dump_handles(o, n, n_det, det)))
    before = _dump_handles(o, n, n_det, det)
    assert o.set_output(o.last(1)) == 1
    exp.append(expected_flagged(before, _dump_handles(o, n, n_det, det)))
    before = _dump_handles(o, n, n_det, det)
    o.invalidate_slots([8], [1])
    exp.append(expected_flagged(before, _dump_handles(o, n, n_det, det)))
    assert np.array_equal(ids, o.inv_log().astype(np.uint32)) and list(ids) == [0, 3, 1]
    assert [list(e[0]) for e in exp] == [[1, 2, 8], [5, 6], [7], [8]]
    for k in range(4):
        assert len(per[k][0]) >= 1, f"step {k} reported nothing"
        _assert_step(per[k], exp[k][0], exp[k][1], f"step {k}")
    # 8 under steps 0 and 3, with different flags
    assert per[0][1][list(per[0][0]).index(8)] == COMPUTING | F_IOSO
    assert list(per[3][0]) == [8] and list(per[3][1]) == [COMPUTING | F_IOSO | F_DS]
    # the Computing own slot is not reported under step 1: its node lives on at out[1] with its flag
    assert 4 not in per[1][0]
    assert g.get_state([int(dh[1])])[1][0] == COMPUTING | F_IOSO
    assert_states_equal(g, o, n)


def test_accessor_contract(pkg, gpu_available):
    fgi = pkg.fgi
    arrays, waves, _ = _mixed()
    g = _engine(pkg, N, *arrays)
    g.run_batch([("invalidate", waves[0][0], waves[0][1])])
    need = len(waves[0][3])
    st_, ids, fl = (np.zeros(need, np.uint32) for _ in range(3))
    n = C.c_uint64()

    def p(a):
        return a.ctypes.data_as(U32P)


    assert g.lib.fgi_last_batch_flagged(g.h, None, None, None, 0, C.byref(n)) == fgi.OK and n.value == need
    n.value = 0
    assert g.lib.fgi_last_batch_flagged(g.h, p(st_), p(ids), p(fl), need - 1, C.byref(n)) == fgi.ECAPACITY
    assert n.value == need
    assert g.lib.fgi_last_batch_flagged(g.h, None, p(ids), None, need, C.byref(n)) == fgi.OK
    assert np.array_equal(ids, waves[0][3])
    assert g.lib.fgi_last_batch_flagged(g.h, p(st_), p(ids), p(fl), need, C.byref(n)) == fgi.OK
    assert np.all(st_ == 0) and np.array_equal(ids, waves[0][3]) and np.array_equal(fl, waves[0][4])
    # the single-wave accessor still does not report a batch
    with pytest.raises(pkg.FgiError) as e:
        g.last_wave_flagged()
    assert e.value.status == fgi.ENOTSUP and "fgi_last_batch_flagged" in str(e.value)
    # a single wave ends the records' validity
    g.invalidate(waves[1][0], waves[1][1])
    with pytest.raises(pkg.FgiError) as e:
        g.last_batch_flagged()
    assert e.value.status == fgi.ENOTSUP
    # the next batch reports itself only
    g.run_batch([("invalidate", waves[2][0], waves[2][1])])
    _assert_step(_by_step(g.last_batch_flagged(), 1)[0], waves[2][3], waves[2][4], "second batch")
    # an empty batch reports nothing
    g.run_batch([])
    assert all(len(a) == 0 for a in g.last_batch_flagged())
    # a graph that cannot flag: no records, no flagged visits
    scale, seed = 10, 0x5EED0024
    r = pkg.Graph(1 << scale)
    r.synth_rmat(scale, 8, seed, 0, 0)
    s, _ = O.gen_rmat(scale, 8, seed)
    roots = O.gen_roots(16, 1 << scale, 0x5EED1024, np.bincount(s, minlength=1 << scale))
    bs = fgi.BatchStats()
    got, _ = r.run_batch([("invalidate", roots)], stats=bs)
    assert len(got) > 16 and bs.n_flagged == 0
    assert all(len(a) == 0 for a in r.last_batch_flagged())


def test_resume_after_pool_growth(pkg, gpu_available):
    """test_batch_grows_the_pool's shape: the add_used step outgrows the pool, the call grows it and resumes
    from that step. The cascade before it (step 0) and the one after (step 4) report what the same calls
    made singly report."""
    n = 3_000_010
    ver = O.version_of(11, np.arange(n))
    flags = np.full(n, CONSISTENT, np.uint32)
    flags[[2, 10]] |= F_HD                  # delayed: 2 under node 1, 10 under node 0
    flags[[3, 11]] = COMPUTING              # Computing: 3 under node 1, 11 under node 0
    src = np.append(np.zeros(n - 10, np.uint32), [1, 1]).astype(np.uint32)
    dst = np.append(np.arange(10, n, dtype=np.uint32), [2, 3]).astype(np.uint32)
    got = []
    for use_batch in (False, True):
        g = pkg.Graph(n, n_detached=16)
        g.register_nodes(np.arange(n, dtype=np.uint32), ver, flags)
        g.load_edges(src, dst, ver[dst])
        if use_batch:
            st = pkg.fgi.BatchStats()
            g.run_batch([("invalidate", [1]), ("begin_compute", [5], [ver[5] + 2]), ("add_used", [5], [0]),
                         ("set_output", [5]), ("invalidate", [0])], stats=st)
            assert st.host_syncs >= 2
            per = _by_step(g.last_batch_flagged(), 5)
            assert all(len(per[k][0]) == 0 for k in (1, 2, 3))
            got.append((per[0], per[4]))
        else:
            g.invalidate([1])
            first = g.last_wave_flagged()
            g.begin_compute([5], [ver[5] + 2])
            g.add_used([5], [0])
            g.set_output([5])
            g.invalidate([0])
            got.append((first, g.last_wave_flagged()))
        g.close()
    single, batch = got
    assert list(single[0][0]) == [2, 3] and list(single[1][0]) == [10, 11]
    for k in range(2):
        _assert_step(batch[k], single[k][0], single[k][1], f"cascade {k}")


def test_out_of_detached_handles(pkg, gpu_available):
    g = pkg.Graph(8, n_detached=1)
    g.register_nodes(np.arange(8, dtype=np.uint32), np.arange(8, dtype=np.uint64) * 2 + 1, np.zeros(8, np.uint32))
    with pytest.raises(pkg.FgiError) as e:
        g.run_batch([("invalidate", [7]), ("begin_compute", [0, 1], [101, 103]), ("invalidate", [6])])
    assert e.value.status == pkg.fgi.ECAPACITY
    steps, ids, fl = g.last_batch_flagged()
    assert list(steps) == [0] and list(ids) == [7] and list(fl) == [COMPUTING | F_IOSO]
    g.close()


def test_partition_reports_nothing(pkg, gpu_available):
    n = 64
    gs, _ = _group(pkg, 2, n)
    slots = np.arange(n, dtype=np.uint32)
    ver = O.version_of(3, slots.astype(np.uint64))
    used, dep = np.array([1, 40], np.uint32), np.array([2, 3], np.uint32)
    for g in gs:
        g.part_register_nodes(slots, ver, np.full(n, CONSISTENT, np.uint32))
        g.part_load_edges(used, dep, ver[dep])
    pkg.fgi.part_local_run_batch(gs, [("invalidate", [1, 40])])
    for g in gs:
        with pytest.raises(pkg.FgiError) as e:
            g.last_batch_flagged()
        assert e.value.status == pkg.fgi.ENOTSUP
