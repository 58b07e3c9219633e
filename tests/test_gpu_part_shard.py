"""A partition loaded from per-rank shards (fgi_part_register_shard / fgi_part_load_edges_shard, C-ABI 0.5):
every rank hands in its own nodes and edges, whoever owns them, and the engine routes them to their owners.
In-process groups (fgi_part_local_register_shards / fgi_part_local_load_shards: the calls on one host thread
per rank, device copies for the collectives) must reproduce the oracle on the committed golden fixtures, and on
random mixed-state graphs everything a twin group loaded through the replicated calls with the concatenation
of the shards holds: rows, node words, two waves and their flagged sets. Also: the partition codes agree when
the heaviest slot is known to one rank only, refusals reach every rank and apply nothing, and world size 1
(in-process, and a real RCCL communicator with and without its collectives)."""
import glob
import json
import os

import numpy as np
import pytest

import fgo as O
from harness import F_DS, F_HD, canon_edges, random_states
from test_gpu_flagged import expected_flagged
from test_gpu_parity import _edges_from_live
from test_gpu_part_load import _check

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.json")))


def _group(pkg, n, P, direction=0, labels=0, tpb=0):
    block = -(-n // P)
    gs = [pkg.Graph(block, rank=r, world=P, labels=labels) for r in range(P)]
    pkg.fgi.part_init_local(gs, n)
    for g in gs:
        g.set_option(pkg.fgi.OPT_DIRECTION, direction)
        if tpb:
            g.set_option(pkg.fgi.OPT_PULL_TPB, tpb)
    return gs, block


def _deal(P, *arrays):
    """Item i to rank i % P: nearly every item then sits on a rank that does not own it."""
    return [tuple(a[r::P] for a in arrays) for r in range(P)]


def _close(*groups):
    for gs in groups:
        for g in gs:
            g.close()


@pytest.mark.parametrize("direction", [1, 0])
@pytest.mark.parametrize("P", [2, 3, 8])
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-5] for p in GOLDEN])
def test_shards_load_golden_fixture(pkg, gpu_available, path, P, direction):
    doc = json.load(open(path))
    n = doc["n_slots"]
    v = np.array(doc["versions"], np.uint64)
    f = np.array(doc["state_flags"], np.uint32)
    u = np.array(doc["used"], np.uint32)
    d = np.array(doc["dependant"], np.uint32)
    t = np.array(doc["tags"], np.uint64)
    gs, block = _group(pkg, n, P, direction)
    present = np.nonzero(v)[0].astype(np.uint32)
    pkg.fgi.part_local_register_shards(gs, _deal(P, present, v[present], f[present]))
    pkg.fgi.part_local_load_shards(gs, _deal(P, u, d, t))
    o = O.Oracle(n)
    o.load_graph(v, f, u, d, t)
    _check(pkg, gs, block, n, o, np.array(doc["roots"], np.uint32), np.array(doc["immediately"], np.uint8))
    ids = np.sort(np.concatenate([g.part_export_ids() for g in gs]))
    assert ids.tolist() == doc["expected"]["inv"]
    _close(gs)
    o.close()


def _uneven(P, block, n, used, dep, tags):
    """Edge shards, uneven on purpose: rank 0's is empty; rank 1 holds about 70% (everything at P = 2); from
    P = 3 on the last rank's edges all have both ends in rank 1's range, so all its records go to one owner, and
    the ranks in between share the rest; no length is made a multiple of 64."""
    m = len(used)
    empty = (used[:0], dep[:0], tags[:0])
    if P == 2:
        return [empty, (used, dep, tags)]
    lo, hi = block, min(n, 2 * block)
    one = (used >= lo) & (used < hi) & (dep >= lo) & (dep < hi)
    rest = np.nonzero(~one)[0]
    cut = min(len(rest), int(0.7 * m) | 1)
    parts = [rest[:0], rest[:cut]] + [rest[cut:][r::P - 3] for r in range(P - 3)] + [np.nonzero(one)[0]]
    if P == 3:   # nobody in between: rank 1 takes the rest too
        parts[1] = rest
    assert len(parts) == P and sum(len(x) for x in parts) == m and len(parts[-1]) > 0
    return [(used[x], dep[x], tags[x]) for x in parts]


def _same_as_twin(pkg, gs, twin, block, n, what):
    for r, (g, w) in enumerate(zip(gs, twin)):
        assert np.array_equal(canon_edges(*g.export_edges()), canon_edges(*w.export_edges())), (what, r, "rows")
        (gv, gf), (wv, wf) = g.dump_states(), w.dump_states()
        assert np.array_equal(gv, wv) and np.array_equal(gf, wf), (what, r, "node words")


def _flagged(gs):
    return [g.part_last_flagged() for g in gs]


@pytest.mark.parametrize("order", ["shard_then_replicated", "replicated_then_shard"])
@pytest.mark.parametrize("labels,tpb", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("direction", [1, 2, 0])
@pytest.mark.parametrize("P", [2, 3, 8])
def test_shards_load_mixed_state_graph(pkg, gpu_available, P, direction, labels, tpb, order):
    """test_partition_loads_mixed_state_graph's graph (n = 4,096; 60,000 + 20,000 edges, 30% stale, 500
    duplicates across the batches), the nodes registered from shards, one batch loaded from uneven shards
    (_uneven) and the other through the replicated call, against a twin group given the concatenations
    through the replicated calls only, and against the oracle."""
    rng = np.random.default_rng(100 + 10 * P + direction)
    n = 4096
    versions, flags = random_states(n, rng)
    src, dst, tags = _edges_from_live(versions, flags, rng, 60000, n, stale_p=0.3)
    src2, dst2, tags2 = _edges_from_live(versions, flags, rng, 20000, n, stale_p=0.3)
    src2 = np.concatenate([src2, src[:500]])
    dst2 = np.concatenate([dst2, dst[:500]])
    tags2 = np.concatenate([tags2, tags[:500]])
    gs, block = _group(pkg, n, P, direction, labels, tpb)
    twin, _ = _group(pkg, n, P, direction, labels, tpb)
    # node shards: dealt unevenly, and one delayed node that rank 0 owns is listed by the last rank only
    present = np.nonzero(versions)[0].astype(np.uint32)
    delayed = present[(present < block) & ((flags[present] & (F_HD | F_DS)) == F_HD) & ((flags[present] & 3) == 1)][0]
    to = (present.astype(np.uint64) * 7 + 3) % P
    to[rng.random(len(present)) < 0.5] = P - 1
    to[present == delayed] = P - 1
    nodes = [present[to == r] for r in range(P)]
    assert delayed in nodes[P - 1] and delayed // block == 0
    pkg.fgi.part_local_register_shards(gs, [(x, versions[x], flags[x]) for x in nodes])
    cat = np.concatenate(nodes)
    for w in twin:
        w.part_register_nodes(cat, versions[cat], flags[cat])
    for k, (u, d, t) in enumerate(((src, dst, tags), (src2, dst2, tags2))):
        shards = _uneven(P, block, n, u, d, t)
        cu, cd, ct = (np.concatenate([s[i] for s in shards]) for i in range(3))
        if (k == 0) == (order == "shard_then_replicated"):
            pkg.fgi.part_local_load_shards(gs, shards)
        else:
            for g in gs:
                g.part_load_edges(cu, cd, ct)
        for w in twin:
            w.part_load_edges(cu, cd, ct)
    _same_as_twin(pkg, gs, twin, block, n, "loaded")
    o = O.Oracle(n)
    o.load_graph(versions, flags, np.concatenate([src, src2]), np.concatenate([dst, dst2]), np.concatenate([tags, tags2]))
    waves = [(rng.integers(0, n, 200).astype(np.uint32), (rng.random(200) < 0.3).astype(np.uint8)),
             (rng.integers(0, n, 64).astype(np.uint32), None)]
    waves[0][0][0] = delayed   # a non-immediate visit of the delayed node only flags it
    waves[0][1][waves[0][0] == delayed] = 0
    for k, (roots, imm) in enumerate(waves):
        before = o.dump_states()
        stats = _check(pkg, gs, block, n, o, roots, imm)
        exp_ids, exp_flags = expected_flagged(before, o.dump_states())
        tstats = pkg.fgi.part_local_invalidate(twin, roots, imm)
        got, want = _flagged(gs), _flagged(twin)
        for r in range(P):
            assert np.array_equal(gs[r].part_export_ids(), twin[r].part_export_ids()), (k, r)
            assert (stats[r].v_inv, stats[r].e_trav) == (tstats[r].v_inv, tstats[r].e_trav), (k, r)
            assert all(np.array_equal(a, b) for a, b in zip(got[r], want[r])), (k, r, "flagged sets")
        ids = np.concatenate([x[1] for x in got])
        fl = np.concatenate([x[2] for x in got])
        assert np.array_equal(ids, exp_ids) and np.array_equal(fl, exp_flags), (k, len(ids), len(exp_ids))
        if k == 0:
            assert len(exp_ids) > 0 and delayed in exp_ids
        _same_as_twin(pkg, gs, twin, block, n, f"wave {k}")
    _close(gs, twin)
    o.close()


def test_shards_codes_agree_from_disjoint_shards(pkg, gpu_available):
    """The inverse of test_partition_codes_disagreement_fails_every_rank: slot 700 (rank 1's) is the heaviest
    dependant, and its registration and every edge touching it are in rank 0's shard only. The weights are
    summed over the ranks before the codes are chosen, so every rank numbers the slots alike and the wave runs."""
    n, P = 1024, 2
    gs, block = _group(pkg, n, P, labels=1)
    versions = O.version_of(1, np.arange(n, dtype=np.uint64))
    rng = np.random.default_rng(7)
    src = rng.integers(0, n, 4000).astype(np.uint32)
    dst = rng.integers(0, n, 4000).astype(np.uint32)
    dst[:600] = 700
    tags = versions[dst]
    slots = np.arange(n, dtype=np.uint32)
    assert 700 // block == 1 and 700 % P == 0   # rank 1 owns it, the deal lists it in rank 0's shard
    pkg.fgi.part_local_register_shards(gs, _deal(P, slots, versions))
    at700 = (src == 700) | (dst == 700)
    e0 = np.nonzero(at700)[0]
    e1 = np.nonzero(~at700)[0]
    pkg.fgi.part_local_load_shards(gs, [(src[e0], dst[e0], tags[e0]), (src[e1], dst[e1], tags[e1])])
    o = O.Oracle(n)
    o.load_graph(versions, None, src, dst, tags)
    _check(pkg, gs, block, n, o, np.array([1, 2, 3, 700], np.uint32), None)
    _close(gs)
    o.close()


def _errors(gs):
    return [(g.lib.fgi_last_error(g.h) or b"").decode() for g in gs]


def test_shard_refusals_reach_every_rank_and_apply_nothing(pkg, gpu_available):
    n, P = 1024, 2
    gs, block = _group(pkg, n, P)
    fgi = pkg.fgi
    u32, u64 = (lambda *a: np.array(a, np.uint32)), (lambda *a: np.array(a, np.uint64))
    # one rank's shard is bad, the other's is fine: both ranks refuse, naming the rank and the item
    bad_nodes = [
        ([(u32(5, 600), u64(3, 9)), (u32(6, n), u64(3, 3))], "rank 1's shard, node 1"),                    # slot out of range
        ([(u32(5, 600), u64(3, 9), u32(1, 3)), (u32(6), u64(3), u32(1))], "rank 0's shard, node 1"),       # state 3
        ([(u32(5), u64(1 << 56)), (u32(6), u64(3))], "rank 0's shard, node 0"),                            # version
    ]
    for shards, what in bad_nodes:
        with pytest.raises(pkg.FgiError) as e:
            fgi.part_local_register_shards(gs, shards)
        assert e.value.status == fgi.EINVAL
        assert all(what in m for m in _errors(gs)), _errors(gs)
    versions = O.version_of(1, np.arange(n, dtype=np.uint64))
    slots = np.arange(n, dtype=np.uint32)
    fgi.part_local_register_shards(gs, _deal(P, slots, versions))   # slots 5, 6, 600 were not installed above
    rng = np.random.default_rng(3)
    src = rng.integers(0, n, 3000).astype(np.uint32)
    dst = rng.integers(0, n, 3000).astype(np.uint32)
    tags = versions[dst]
    bad_edges = [
        ([(src[:10], dst[:10], tags[:10]), (u32(5, 7), u32(700, 9), u64(4, 0))], "rank 1's shard, edge 1"),   # tag 0
        ([(u32(5, n + 3), u32(700, 9), u64(4, 4)), (src[:0], dst[:0], tags[:0])], "rank 0's shard, edge 1"),  # used range
        ([(src[:0], dst[:0], tags[:0]), (u32(5), u32(0xFFFFFFFF), u64(4))], "rank 1's shard, edge 0"),        # dependant
    ]
    for shards, what in bad_edges:
        with pytest.raises(pkg.FgiError) as e:
            fgi.part_local_load_shards(gs, shards)
        assert e.value.status == fgi.EINVAL
        assert all(what in m for m in _errors(gs)), _errors(gs)
    for g in gs:
        assert len(g.export_edges()[0]) == 0   # the good edges of the refused calls were not applied either
    fgi.part_local_load_shards(gs, _deal(P, src, dst, tags))
    o = O.Oracle(n)
    o.load_graph(versions, None, src, dst, tags)
    _check(pkg, gs, block, n, o, rng.integers(0, n, 20).astype(np.uint32), None)
    _close(gs)
    o.close()


def test_shard_registration_of_one_slot_twice_fails_every_rank(pkg, gpu_available):
    n, P = 1024, 2
    gs, _ = _group(pkg, n, P)
    with pytest.raises(pkg.FgiError) as e:   # slot 700 in both shards
        pkg.fgi.part_local_register_shards(gs, [(np.array([5, 700], np.uint32), np.array([3, 9], np.uint64)),
                                                (np.array([700], np.uint32), np.array([9], np.uint64))])
    assert e.value.status == pkg.fgi.ESTATE
    assert all("already had a current node" in m for m in _errors(gs)), _errors(gs)
    with pytest.raises(pkg.FgiError) as e:   # slot 5 holds a current node since the call above
        pkg.fgi.part_local_register_shards(gs, [(np.array([], np.uint32), np.array([], np.uint64)),
                                                (np.array([5], np.uint32), np.array([7], np.uint64))])
    assert e.value.status == pkg.fgi.ESTATE
    assert all("already had a current node" in m for m in _errors(gs)), _errors(gs)
    _close(gs)


def test_shard_calls_refuse_a_graph_that_is_not_partitioned(pkg, gpu_available):
    g = pkg.Graph(256)
    with pytest.raises(pkg.FgiError) as e:
        g.part_register_shard(np.array([1], np.uint32), np.array([3], np.uint64))
    assert e.value.status == pkg.fgi.ESTATE
    with pytest.raises(pkg.FgiError) as e:
        g.part_load_edges_shard(np.array([1], np.uint32), np.array([2], np.uint32), np.array([3], np.uint64))
    assert e.value.status == pkg.fgi.ESTATE
    g.close()


def _rmat11():
    scale, ef, seed, sseed = 11, 8, 0x5EED0027, 0x5EED00C0
    n = 1 << scale
    s, d = O.gen_rmat(scale, ef, seed)
    return n, O.version_of(seed, np.arange(n)), s, d, O.gen_tags(s, d, seed, 50, sseed)


def test_shards_world1_in_process_group(pkg, gpu_available):
    n, versions, s, d, tags = _rmat11()
    gs, block = _group(pkg, n, 1)
    pkg.fgi.part_local_register_shards(gs, [(np.arange(n, dtype=np.uint32), versions)])
    pkg.fgi.part_local_load_shards(gs, [(s, d, tags)])
    o = O.Oracle(n)
    o.load_graph(versions, None, s, d, tags)
    _check(pkg, gs, block, n, o, O.gen_roots(48, n, 0x5EED1027, np.bincount(s, minlength=n)), None)
    _close(gs)
    o.close()


@pytest.mark.parametrize("collectives", [1, 0])
def test_shards_world1_rccl(pkg, gpu_available, collectives):
    """The RCCL transport of the two calls at world size 1: with FGI_OPT_PART_COLLECTIVES the counts, the
    records and the weight blocks go through the communicator (grouped send / receive to itself)."""
    import torch
    n, versions, s, d, tags = _rmat11()
    g = pkg.Graph(n, rank=0, world=1)
    g.part_init(n, pkg.fgi.part_unique_id())
    g.set_option(pkg.fgi.OPT_PART_COLLECTIVES, collectives)
    g.part_register_shard(np.arange(n, dtype=np.uint32), versions)
    g.part_load_edges_shard(s, d, tags)
    o = O.Oracle(n)
    o.load_graph(versions, None, s, d, tags)
    roots = O.gen_roots(48, n, 0x5EED1027, np.bincount(s, minlength=n))
    st = o.invalidate_slots(roots, None)
    d_roots = torch.from_numpy(roots.astype(np.int32)).cuda()
    stats = pkg.fgi.WaveStats()
    n_inv = g.part_invalidate(len(roots), d_roots.data_ptr(), 0, stats)
    ids = g.part_export_ids()
    assert n_inv == len(ids) == st.v_inv and stats.e_trav == st.e_trav
    assert np.array_equal(np.sort(ids), np.sort(o.inv_log()))
    ov, of = o.dump_states()
    v, f = g.dump_states()
    assert np.array_equal(v[:n], ov) and np.array_equal(f[:n], of)
    g.close()
    o.close()
