"""fgi_wave_stats on every wave driver: the byte model and the counters as identities and closed forms.

The other tests assert v_inv, e_trav, e_match and a few host_syncs bounds. This file asserts the fields
the drivers tally on the host and fill at the wave's end: alg_bytes (20 B per traversed push edge + 40 B
per frontier entry + the pull levels' bytes + 4 B per invalidated node + 5 B per root, + 8 B per remote
message on a partition), its split into expand_bytes / fused_push_bytes / pull_bytes, f_total and the
launch counts. No recorded numbers: a ring's counters are exact, the rest are sums that must close.
"""
import numpy as np
import pytest

import fgo as O
from harness import CONSISTENT

pytestmark = pytest.mark.gpu


def _ring(pkg, n):
    """A cycle i -> (i + 1) % n with a self loop on every 10th node, all tags live."""
    versions = O.version_of(5, np.arange(n))
    flags = np.full(n, CONSISTENT, np.uint32)
    src = np.arange(n, dtype=np.uint32)
    dst = ((src + 1) % n).astype(np.uint32)
    loops = np.arange(0, n, 10, dtype=np.uint32)
    src = np.concatenate([src, loops])
    dst = np.concatenate([dst, loops])
    g = pkg.Graph(n)
    g.register_nodes(np.arange(n, dtype=np.uint32), versions, flags)
    g.load_edges(src, dst, versions[dst])
    return g


def _assert_ring(ws, n, sync, push_only, what):
    d = ws.as_dict()
    got = (ws.v_inv, ws.levels, ws.f_total, ws.e_trav, ws.roots)
    assert got == (n, n, n, n + n // 10, 1), (what, d)
    if push_only:
        push = 20 * ws.e_trav + 40 * ws.f_total
        assert ws.pull_levels == ws.pull_edges == ws.pull_bytes == 0, (what, d)
        assert ws.alg_bytes == push + 4 * ws.v_inv + 5 * ws.roots, (what, d)
        if sync:
            assert ws.expand_bytes + ws.fused_push_bytes == push, (what, d)
    if sync:
        assert ws.alg_bytes == ws.expand_bytes + ws.fused_push_bytes + ws.pull_bytes + 4 * ws.v_inv + 5 * ws.roots, (what, d)
        assert ws.kernel_ms > 0 and ws.total_ms >= ws.kernel_ms, (what, d)


# 40 levels stay inside the 64-entry level ring (the host's per-level tally); 200 go past it (the
# device's totals, and no directions kept for the next wave's plan)
@pytest.mark.parametrize("level_timing", [None, 0])   # the wave's span from stream events / the device clock
@pytest.mark.parametrize("n", [40, 200])
def test_ring_wave_stats_are_exact(pkg, gpu_available, n, level_timing):
    """Three synchronous waves (level groups without the tail, then twice through the tail) and two
    asynchronous ones, each from the snapshot.

    The 40-node ring is not push-only in automatic direction: Beamer's alpha rule pulls a level of more
    than edges / 28 frontier edges, which is 1 for 44 edges, so the levels of the four self-loop nodes
    (2 edges) pull once the dependency lists exist. Measured: 3 pull levels in the first wave (pull_edges
    51, pull_bytes 2,032, alg_bytes 4,437), 4 in the repeats (pull_bytes 3,172, alg_bytes 5,497, 4 host
    synchronisations) and 1 in the asynchronous waves with 3 more pushed inside the tail (pull_pushed 3,
    alg_bytes 3,787). So at n = 40 the push-only closed forms and the repeats' single synchronisation
    are not asserted; the exact counters and the closing sum are. At n = 200 (threshold 7) no level pulls
    and everything is asserted."""
    import torch
    push_only = n == 200
    g = _ring(pkg, n)
    if level_timing is not None:
        g.set_option(pkg.fgi.OPT_LEVEL_TIMING, level_timing)
    g.snapshot()
    roots = np.array([17], np.uint32)
    for rep in range(3):
        g.restore()
        ws = pkg.WaveStats()
        ids = g.invalidate(roots, stats=ws)
        assert len(ids) == n
        _assert_ring(ws, n, True, push_only, ("sync", rep))
        if rep == 0:
            assert ws.fused_launches == 0, ws.as_dict()
        else:
            assert ws.fused_launches >= 1, ws.as_dict()
            if push_only:
                assert ws.host_syncs == 1, ws.as_dict()
    if level_timing is None:
        d_roots = torch.from_numpy(roots.astype(np.int32)).cuda()
        torch.cuda.synchronize()
        for rep in range(2):
            g.restore()
            ws = pkg.WaveStats()
            nv, _ = g.wave_wait(g.invalidate_async(1, d_roots.data_ptr()), ws)
            assert nv == n
            _assert_ring(ws, n, False, push_only, ("async", rep))
    g.close()


SCALE, EF, SEED, STALE, SSEED = 12, 8, 0x5EED0024, 50, 0x5EED00C0


@pytest.fixture(scope="module")
def rmat_ref():
    """The oracle's wave on the R-MAT graph, once: (roots, V_inv, E_trav)."""
    n = 1 << SCALE
    s, d = O.gen_rmat(SCALE, EF, SEED)
    o = O.Oracle(n)
    o.load_graph(O.version_of(SEED, np.arange(n)), None, s, d, O.gen_tags(s, d, SEED, STALE, SSEED))
    roots = O.gen_roots(64, n, 0x5EED1024, np.bincount(s, minlength=n))
    st = o.invalidate_slots(roots)
    o.close()
    return roots, st.v_inv, st.e_trav


def test_pull_wave_bytes_close(pkg, gpu_available, rmat_ref):
    roots, v_inv, e_trav = rmat_ref
    g = pkg.Graph(1 << SCALE)
    g.set_option(pkg.fgi.OPT_DIRECTION, 2)
    g.synth_rmat(SCALE, EF, SEED, STALE, SSEED)
    ws = pkg.WaveStats()
    g.invalidate(roots, stats=ws)
    d = ws.as_dict()
    assert (ws.v_inv, ws.e_trav) == (v_inv, e_trav), d
    assert ws.alg_bytes == ws.expand_bytes + ws.fused_push_bytes + ws.pull_bytes + 4 * ws.v_inv + 5 * ws.roots, d
    assert ws.pull_bytes > 0, d
    assert ws.pull_levels == ws.levels, d
    g.close()


@pytest.mark.parametrize("plan", [1, 0])   # the planned path (its second wave) / the host-driven levels
def test_partitioned_wave_bytes_close(pkg, gpu_available, rmat_ref, plan):
    roots, v_inv, e_trav = rmat_ref
    P, n = 2, 1 << SCALE
    gs = [pkg.Graph(n // P, rank=r, world=P) for r in range(P)]
    pkg.fgi.part_init_local(gs, n)
    for g in gs:
        g.part_synth_rmat(SCALE, EF, SEED, STALE, SSEED)
        if not plan:
            g.set_option(pkg.fgi.OPT_PART_PLAN, 0)
        g.snapshot()
    for rep in range(2 if plan else 1):
        for g in gs:
            g.restore()
        stats = pkg.fgi.part_local_invalidate(gs, roots)
        ds = [x.as_dict() for x in stats]
        for x in stats:
            assert x.alg_bytes == x.expand_bytes + x.pull_bytes + 4 * x.v_inv + 8 * x.remote_msgs + 5 * x.roots, (rep, ds)
        assert sum(x.v_inv for x in stats) == v_inv, (rep, ds)
        assert sum(x.e_trav for x in stats) == e_trav, (rep, ds)
        if plan and rep:   # the wave followed the plan: the start's and the closing all-reduce only
            assert all(x.host_syncs == 2 for x in stats), ds
    for g in gs:
        g.close()
