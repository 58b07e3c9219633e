"""The pull candidates' packed records and the tail runs they point into.

A candidate's 16-byte record holds its slot relative to its pull block, the tail flag, a 20-bit row
length (all ones: read the row table) and a 28-bit offset of its tail run (all ones: locate the list
through the per-slot offsets), and a tail scan reads [length, entry 2, entry 3, ...] from that run. These
tests walk the edges of that layout: every list length at which the tail scan changes pass, survivors
re-read at later pull levels, both escapes, a rebuilt cache and a partition — each against the oracle.
"""
import numpy as np
import pytest

import fgo as O
from harness import CONSISTENT, assert_states_equal, build_pair

pytestmark = pytest.mark.gpu

PULL = 2   # FGI_OPT_DIRECTION: every level pulls


def _wave(pkg, g, roots):
    ws = pkg.WaveStats()
    ids = g.invalidate(roots, stats=ws)
    return np.sort(ids), ws


def _oracle_wave(o, roots):
    o.clear_log()
    st = o.invalidate_slots(roots)
    return np.sort(o.inv_log()), st.v_inv, st.e_trav


# ---- 1. list-length boundaries ---------------------------------------------------------------------
# Lists are ordered by their entries' own list lengths, descending. Every filler parent has one parent
# of its own (Z), the roots have none, so a root is the last entry of each list it is in.
LENGTHS = [1, 2, 3, 4, 5, 12, 13, 20, 5000]
N1 = 6144                       # six pull tiles
R, Z, R5 = 0, 1, 2              # the root; the fillers' parent; the last parent of the 5,000-entry list
FILL0 = 10
CAND0, CAND_STEP = 5100, 100    # candidates in tiles 4 and 5
D1, D2 = 6000, 6100             # a chain below the 1-entry candidate: two more pull levels


def _boundary_graph():
    src, dst = [], []
    n_fill = max(LENGTHS) - 1
    fill = np.arange(FILL0, FILL0 + n_fill, dtype=np.uint32)
    src.append(np.full(n_fill, Z, np.uint32))
    dst.append(fill)
    for i, ln in enumerate(LENGTHS):
        c = CAND0 + CAND_STEP * i
        last = R5 if ln == 5000 else R
        src.append(np.concatenate([fill[:ln - 1], np.array([last], np.uint32)]))
        dst.append(np.full(ln, c, np.uint32))
    src.append(np.array([CAND0, D1], np.uint32))
    dst.append(np.array([D1, D2], np.uint32))
    src, dst = np.concatenate(src), np.concatenate(dst)
    versions = O.version_of(77, np.arange(N1))
    flags = np.full(N1, CONSISTENT, np.uint32)
    return versions, flags, src, dst, versions[dst]


@pytest.fixture(scope="module")
def boundary_ref():
    """The graph and the oracle's two waves: with both roots, and without the long list's."""
    versions, flags, src, dst, tags = _boundary_graph()
    o = O.Oracle(N1)
    o.load_graph(versions, flags, src, dst, tags)
    o.snapshot()
    ref = {}
    for name, roots in (("hit", [R, R5]), ("survive", [R])):
        o.restore()
        ref[name] = (np.array(roots, np.uint32),) + _oracle_wave(o, np.array(roots, np.uint32))
    o.close()
    return (versions, flags, src, dst, tags), ref


def test_list_length_boundaries(pkg, gpu_available, boundary_ref):
    (versions, flags, src, dst, tags), ref = boundary_ref
    cands = {CAND0 + CAND_STEP * i for i in range(len(LENGTHS))}
    assert cands | {D1, D2, R, R5} == set(ref["hit"][1].tolist())
    assert cands - {CAND0 + CAND_STEP * (len(LENGTHS) - 1)} | {D1, D2, R} == set(ref["survive"][1].tolist())
    seen = {}
    for tpb in (0, 1, 32):
        g = pkg.Graph(N1)
        g.register_nodes(np.arange(N1, dtype=np.uint32), versions, flags)
        g.load_edges(src, dst, tags)
        g.set_option(pkg.fgi.OPT_DIRECTION, PULL)
        g.set_option(pkg.fgi.OPT_PULL_TPB, tpb)
        g.snapshot()
        for name, (roots, oids, v_inv, e_trav) in ref.items():
            g.restore()
            ids, ws = _wave(pkg, g, roots)
            d = ws.as_dict()
            assert np.array_equal(ids, oids), (name, tpb)
            assert (ws.v_inv, ws.e_trav) == (v_inv, e_trav), (name, tpb, d)
            assert ws.pull_levels == ws.levels >= 3, (name, tpb, d)   # the survivor is re-read twice
            # the survivor and queued-candidate counts reach the statistics through the byte model
            # (16 B each in pull_bytes, beside 16.25 B per candidate scanned and 4 B per tail entry
            # examined, which pull_edges counts): equal on every grid
            seen.setdefault(name, []).append((ws.levels, ws.pull_edges, ws.pull_bytes, ws.n_flagged))
        g.close()
    for name, rows in seen.items():
        assert all(r == rows[0] for r in rows), (name, rows)


# ---- 2. R-MAT, survivors forwarded and re-read -----------------------------------------------------
SCALE, EF, SEED, STALE, SSEED = 12, 8, 0x5EED0024, 50, 0x5EED00C0


@pytest.fixture(scope="module")
def rmat_ref():
    """The oracle's wave on the R-MAT graph, once: (roots, sorted ids, V_inv, E_trav)."""
    n = 1 << SCALE
    s, d = O.gen_rmat(SCALE, EF, SEED)
    o = O.Oracle(n)
    o.load_graph(O.version_of(SEED, np.arange(n)), None, s, d, O.gen_tags(s, d, SEED, STALE, SSEED))
    roots = O.gen_roots(64, n, 0x5EED1024, np.bincount(s, minlength=n))
    ids, v_inv, e_trav = _oracle_wave(o, roots)
    o.close()
    return roots, ids, v_inv, e_trav


@pytest.mark.parametrize("tpb", [0, 1, 32])
@pytest.mark.parametrize("direction", [0, 2])
def test_rmat_three_waves(pkg, gpu_available, rmat_ref, direction, tpb):
    roots, oids, v_inv, e_trav = rmat_ref
    g = pkg.Graph(1 << SCALE)
    g.set_option(pkg.fgi.OPT_DIRECTION, direction)
    g.set_option(pkg.fgi.OPT_PULL_TPB, tpb)
    g.synth_rmat(SCALE, EF, SEED, STALE, SSEED)
    g.snapshot()
    for rep in range(3):
        g.restore()
        ids, ws = _wave(pkg, g, roots)
        assert np.array_equal(ids, oids), rep
        assert (ws.v_inv, ws.e_trav) == (v_inv, e_trav), (rep, ws.as_dict())
        if direction == PULL:
            assert ws.pull_levels == ws.levels and ws.pull_bytes > 0, (rep, ws.as_dict())
    g.close()


# ---- 3. the row-length escape ----------------------------------------------------------------------
def test_row_length_escape(pkg, gpu_available):
    """Winners of a pull level whose rows hold 2^20 - 2 (the field's largest length), 2^20 - 1 (the
    escape value itself) and 2^20 entries: their row lengths are the next level's edge count."""
    big = 1 << 20
    hubs = [(1, big), (2, big - 1), (3, big - 2)]
    n = big + 16
    dep = np.arange(16, 16 + big, dtype=np.uint32)
    src = [np.zeros(len(hubs), np.uint32)]
    dst = [np.array([h for h, _ in hubs], np.uint32)]
    for h, k in hubs:
        src.append(np.full(k, h, np.uint32))
        dst.append(dep[:k])
    src, dst = np.concatenate(src), np.concatenate(dst)
    versions = O.version_of(31, np.arange(n))
    flags = np.full(n, CONSISTENT, np.uint32)
    g, o = build_pair(pkg, n, versions, flags, src, dst, versions[dst])
    g.set_option(pkg.fgi.OPT_DIRECTION, PULL)
    roots = np.array([0], np.uint32)
    oids, v_inv, e_trav = _oracle_wave(o, roots)
    ids, ws = _wave(pkg, g, roots)
    assert e_trav == len(src) and v_inv == big + 4
    assert (ws.v_inv, ws.e_trav) == (v_inv, e_trav), ws.as_dict()
    assert np.array_equal(ids, oids)
    assert ws.pull_levels == ws.levels >= 2, ws.as_dict()
    g.close()
    o.close()


# ---- 4. the offset escape --------------------------------------------------------------------------
@pytest.mark.parametrize("tpb", [0, 32])
@pytest.mark.parametrize("bits", [8, 1])
def test_run_offset_escape(pkg, gpu_available, rmat_ref, bits, tpb):
    """With the inline offset cut to 2^8 words (2^1: every run but a block's first) most candidates
    carry no offset and are located through uin_len / uin_off: same results, same counters."""
    roots, oids, v_inv, e_trav = rmat_ref
    rows = []
    for b in (bits, 28):
        g = pkg.Graph(1 << SCALE)
        g.set_option(pkg.fgi.OPT_DIRECTION, PULL)
        g.set_option(pkg.fgi.OPT_PULL_TPB, tpb)
        g.set_option(pkg.fgi.OPT_RUN_OFFSET_BITS, b)
        g.synth_rmat(SCALE, EF, SEED, STALE, SSEED)
        g.snapshot()
        for rep in range(2):
            g.restore()
            ids, ws = _wave(pkg, g, roots)
            assert np.array_equal(ids, oids), (b, rep)
            assert (ws.v_inv, ws.e_trav) == (v_inv, e_trav), (b, rep, ws.as_dict())
            rows.append((ws.levels, ws.pull_levels, ws.pull_edges, ws.pull_bytes, ws.n_flagged))
        g.close()
    assert all(r == rows[0] for r in rows), rows


def test_run_offset_bits_range(pkg, gpu_available):
    g = pkg.Graph(64)
    for bad in (0, 29):
        with pytest.raises(pkg.FgiError):
            g.set_option(pkg.fgi.OPT_RUN_OFFSET_BITS, bad)
    g.close()


# ---- 5. the cache rebuilt after mutations ----------------------------------------------------------
def test_cache_rebuild_after_mutations(pkg, gpu_available):
    """Pull waves between compute-method batches: recomputed nodes drop their old dependency lists
    (shorter: one dependency; longer: nine) and the next pull wave reads rebuilt records and runs."""
    from test_gpu_parity import Pair
    rng = np.random.default_rng(61)
    n = 3000
    p = Pair(pkg, n, n_detached=8192)
    p.g.set_option(pkg.fgi.OPT_DIRECTION, PULL)
    ver = O.version_of(23, np.arange(n))
    slots = np.arange(n, dtype=np.uint32)
    p.begin(slots, ver, np.zeros(n, np.uint8))
    p.g.set_output(slots)
    for s_ in slots:
        p.o.set_output(p.node(int(s_)))
    for step, per in enumerate((4, 9, 1, 6)):
        batch = rng.choice(n, 1200, replace=False).astype(np.uint32)
        ver[batch] += np.uint64(1000)
        p.begin(batch, ver[batch], np.zeros(len(batch), np.uint8))
        dep = np.repeat(batch, per)
        use = ((rng.integers(0, n, len(batch))[:, None] + 7 * np.arange(per)[None, :]) % n).astype(np.uint32).ravel()
        res = p.g.add_used(dep, use)
        assert list(res) == [p.o.add_used(p.node(int(d)), p.node(int(u))) for d, u in zip(dep, use)]
        p.g.set_output(batch)
        for s_ in batch:
            p.o.set_output(p.node(int(s_)))
        # the invalidated set and the node states, as the other compute-method tests compare them
        # (E_trav is left out: after recomputations the engine's and the oracle's counts differ, with the
        # previous record layout as well)
        roots = rng.choice(n, 20, replace=False).astype(np.uint32)
        oids, v_inv, _ = _oracle_wave(p.o, roots)
        ids, ws = _wave(pkg, p.g, roots)
        assert np.array_equal(ids, oids), step
        assert ws.v_inv == v_inv and ws.pull_levels == ws.levels, (step, ws.as_dict())
        assert_states_equal(p.g, p.o, n)
    p.g.close()
    p.o.close()


# ---- 6. a two-rank partition -----------------------------------------------------------------------
def test_two_rank_partition_pull(pkg, gpu_available, rmat_ref):
    roots, _, v_inv, e_trav = rmat_ref
    P, n = 2, 1 << SCALE
    gs = [pkg.Graph(n // P, rank=r, world=P) for r in range(P)]
    pkg.fgi.part_init_local(gs, n)
    for g in gs:
        g.set_option(pkg.fgi.OPT_DIRECTION, PULL)
        g.part_synth_rmat(SCALE, EF, SEED, STALE, SSEED)
        g.snapshot()
    for rep in range(2):
        for g in gs:
            g.restore()
        stats = pkg.fgi.part_local_invalidate(gs, roots)
        ds = [x.as_dict() for x in stats]
        assert sum(x.v_inv for x in stats) == v_inv, (rep, ds)
        assert sum(x.e_trav for x in stats) == e_trav, (rep, ds)
        assert all(x.pull_levels > 0 and x.pull_bytes > 0 for x in stats), (rep, ds)
    for g in gs:
        g.close()
