"""A partition's host-facing wave (C-ABI 0.8) against the CPU oracle: fgi_part_invalidate_host /
fgi_part_invalidate_bits (host roots in) and fgi_part_last_wave_ids / fgi_part_last_wave_bits /
fgi_part_wave_ids_dev (this rank's share of its last wave, made on the device in the host's numbering).

A rank's ids are the global slots it owns that the wave moved from Consistent to Invalidated
(Computed.cs:162-230), strictly ascending; its bitmap is addressed like the planes of its state view (bit h =
global slot rank * block + h), every other bit 0. With labels = 1 the ranks' engines run on partition codes,
so both are renumbered on the device: FGI_OPT_PART_IDS_PATH pins the scatter (1) and the gather (2) form on
these small graphs, 0 leaves the choice to the wave's size."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fgo as O
from harness import CONSISTENT
from test_gpu_async import _d2h
from test_gpu_flagged import N, _engine, _mixed
from test_gpu_part_host import _free_port
from test_gpu_part_state_view import _build_with, _open

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import part_host_roots_worker as RW  # noqa: E402

# (labels, FGI_OPT_PART_IDS_PATH): without codes the bitmap is the engine's own; with codes both forms pinned,
# and the automatic choice
CODES = [(0, 0), (1, 1), (1, 2), (1, 0)]
PINNED = [(0, 0), (1, 1), (1, 2)]


def _range(r, block, n):
    return r * block, min(n, (r + 1) * block)


def _expect_bits(g, ids, lo):
    bits = np.zeros((g.n_handles + 63) // 64, np.uint64)
    h = (ids - lo).astype(np.int64)
    np.bitwise_or.at(bits, h >> 6, np.uint64(1) << (h & 63).astype(np.uint64))
    return bits


def _check_rank(pkg, g, r, block, n, inv, what):
    """Rank r's three accessors against the oracle's invalidated set `inv` (ascending global slots)."""
    lo, hi = _range(r, block, n)
    want = inv[(inv >= lo) & (inv < hi)].astype(np.uint32)
    bits, nb = g.part_last_wave_bits()
    assert nb == len(want), f"{what}, rank {r}: V_inv {nb} vs oracle {len(want)}"
    assert np.array_equal(bits, _expect_bits(g, want, lo)), f"{what}, rank {r}: bitmap differs"
    assert np.array_equal(pkg.fgi.bits_to_ids(bits) + np.uint32(lo), want), f"{what}, rank {r}: decoded bitmap"
    ids = g.part_last_wave_ids()
    assert np.all(np.diff(ids.astype(np.int64)) > 0), f"{what}, rank {r}: ids not strictly ascending"
    assert np.array_equal(ids, want), f"{what}, rank {r}: ids differ ({len(ids)} vs {len(want)})"
    ptr, nd = g.part_wave_ids_dev()
    assert nd == len(want) and np.array_equal(_d2h(ptr, nd), want), f"{what}, rank {r}: device list differs"
    return want


def _chain(pkg, labels, path, n=200, P=3, n_det=8):
    versions = O.version_of(11, np.arange(n, dtype=np.uint64)).copy()
    flags = np.full(n, CONSISTENT, np.uint32)
    src, dst = np.arange(n - 1, dtype=np.uint32), np.arange(1, n, dtype=np.uint32)
    gs, block = _build_with(pkg, P, n, versions, flags, src, dst, versions[dst],
                            options={pkg.fgi.OPT_PART_IDS_PATH: path}, labels=labels, n_detached=n_det)
    return gs, block, n


# ---- 1. edge shapes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("labels,path", PINNED)
def test_chain_edge_shapes(pkg, gpu_available, labels, path):
    """0 -> 1 -> ... -> 199 over three ranks: block 67, the last rank owns 66 slots, no rank's slot count is a
    multiple of 64, 8 detached handles behind the slots."""
    gs, block, n = _chain(pkg, labels, path)
    assert block == 67 and n - 2 * block == 66 and all(g.n_handles == 75 for g in gs)
    for g in gs:
        g.snapshot()
    # before any wave: nothing, from every accessor
    for r, g in enumerate(gs):
        _check_rank(pkg, g, r, block, n, np.zeros(0, np.uint32), "before any wave")
    pkg.fgi.part_local_invalidate(gs, [0])
    for r, g in enumerate(gs):
        lo, hi = _range(r, block, n)
        got = _check_rank(pkg, g, r, block, n, np.arange(n, dtype=np.uint32), "root 0")
        assert np.array_equal(got, np.arange(lo, hi, dtype=np.uint32))
        bits, _ = g.part_last_wave_bits()
        # exactly the owned bits: the bits past slot 199 and the detached handles' bits are 0
        assert [int(b) for b in bits] == [(1 << 64) - 1, (1 << (hi - lo - 64)) - 1]
    for g in gs:
        g.restore()
    pkg.fgi.part_local_invalidate(gs, [134])   # the first slot of rank 2
    for r, g in enumerate(gs):
        _check_rank(pkg, g, r, block, n, np.arange(134, n, dtype=np.uint32), "root 134")
    assert len(gs[0].part_last_wave_ids()) == 0 and len(gs[1].part_last_wave_ids()) == 0
    assert not gs[0].part_last_wave_bits()[0].any() and not gs[1].part_last_wave_bits()[0].any()
    for g in gs:
        g.restore()
    pkg.fgi.part_local_invalidate(gs, [])
    for r, g in enumerate(gs):
        _check_rank(pkg, g, r, block, n, np.zeros(0, np.uint32), "no roots")
    for g in gs:
        g.close()


# ---- 2. mixed states against the oracle --------------------------------------------------------------------

@pytest.mark.parametrize("labels,path", CODES)
@pytest.mark.parametrize("direction", [0, 1, 2])
@pytest.mark.parametrize("P", [2, 3, 8])
def test_three_mixed_waves(pkg, gpu_available, P, direction, labels, path):
    arrays, waves, _ = _mixed()
    # one pull tile per block, set before the load that chooses the codes (test_gpu_part_state_view.py)
    gs, block = _build_with(pkg, P, N, *arrays, options={pkg.fgi.OPT_PULL_TPB: 1, pkg.fgi.OPT_PART_IDS_PATH: path},
                            direction=direction, labels=labels)
    for k, (roots, imm, inv, *_rest) in enumerate(waves):
        pkg.fgi.part_local_invalidate(gs, roots, imm)
        for r, g in enumerate(gs):
            want = _check_rank(pkg, g, r, block, N, inv, f"wave {k}")
            assert np.array_equal(np.sort(g.part_export_ids()), want), f"wave {k}, rank {r}: part_export_ids"
    for g in gs:
        g.close()


# ---- 3. planned waves and small buckets --------------------------------------------------------------------

@pytest.mark.parametrize("labels,path", PINNED)
@pytest.mark.parametrize("P", [2, 4])
def test_planned_waves_and_small_buckets(pkg, gpu_available, P, labels, path):
    """The same roots three times (the later waves follow the first one's plan), then buckets of one id per
    peer, whose wave repeats its final collect: the invalidated bitmap and the list still stand behind the
    last one."""
    arrays, waves, _ = _mixed()
    gs, block = _build_with(pkg, P, N, *arrays, options={pkg.fgi.OPT_PULL_TPB: 1, pkg.fgi.OPT_PART_IDS_PATH: path},
                            labels=labels)
    for g in gs:
        g.snapshot()
    roots, imm, inv, *_rest = waves[0]
    for what in ("host-driven", "planned", "planned again", "planned, small buckets"):
        if what.endswith("buckets"):
            for g in gs:
                g.set_option(pkg.fgi.OPT_PART_BUCKET, 2)
        print(f"P={P} labels={labels} path={path}: {what}")   # shown if the wave below is refused
        stats = pkg.fgi.part_local_invalidate(gs, roots, imm)
        if what == "planned again":
            assert all(x.host_syncs == 2 for x in stats), [x.host_syncs for x in stats]
        for r, g in enumerate(gs):
            _check_rank(pkg, g, r, block, N, inv, what)
        for r, g in enumerate(gs):
            g.restore()
            _check_rank(pkg, g, r, block, N, np.zeros(0, np.uint32), what + ", restored")
    for g in gs:
        g.close()


# ---- 4. fgi_part_invalidate_host itself --------------------------------------------------------------------

def _world_one(pkg, labels, coll, arrays):
    gs, block = _build_with(pkg, 1, N, *arrays, options={pkg.fgi.OPT_PART_COLLECTIVES: coll}, labels=labels)
    return gs[0]


@pytest.mark.parametrize("coll", [0, 1])
@pytest.mark.parametrize("labels", [0, 1])
def test_invalidate_host_world_one(pkg, gpu_available, labels, coll):
    arrays, waves, o_end = _mixed()
    g = _world_one(pkg, labels, coll, arrays)
    single = _engine(pkg, N, *arrays, labels=-1)
    for k, (roots, imm, inv, *_rest) in enumerate(waves):
        st = pkg.WaveStats()
        if k == 1:
            bits, nv = g.part_invalidate_host(roots, imm, st, want="bits")
            ids = pkg.fgi.bits_to_ids(bits)
            assert nv == len(inv)
        elif k == 2:
            assert g.part_invalidate_host(roots, imm, st, want=None) == len(inv)
            ids = g.part_last_wave_ids()
        else:
            ids = g.part_invalidate_host(roots, imm, st)
        assert st.v_inv == len(inv)
        assert np.array_equal(ids, inv), f"wave {k}: ids differ from the oracle's"
        assert np.array_equal(ids, single.invalidate(roots, imm)), f"wave {k}: ids differ from fgi_invalidate's"
        _check_rank(pkg, g, 0, N, N, inv, f"wave {k}")
    ov, of = o_end.dump_states()
    v, f = g.dump_states()
    assert np.array_equal(v[:N], ov) and np.array_equal(f[:N], of)
    single.close()
    g.close()


@pytest.mark.parametrize("labels", [0, 1])
def test_invalidate_host_refusals(pkg, gpu_available, labels):
    arrays, waves, _ = _mixed()
    g = _world_one(pkg, labels, 0, arrays)
    lib = g.lib
    roots, imm, inv, *_rest = waves[0]
    before = g.dump_states()
    n = C.c_uint64(77)
    # a root equal to n_global: refused, nothing changes
    bad = np.append(roots, np.uint32(N)).astype(np.uint32)
    buf = np.zeros(N, np.uint32)
    st = lib.fgi_part_invalidate_host(g.h, len(bad), bad.ctypes.data_as(C.POINTER(C.c_uint32)), None,
                                      buf.ctypes.data_as(C.POINTER(C.c_uint32)), len(buf), C.byref(n), None)
    assert st == pkg.fgi.EINVAL
    after = g.dump_states()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # a bitmap one word short: refused
    words = (g.n_handles + 63) // 64
    bits = np.zeros(words, np.uint64)
    st = lib.fgi_part_invalidate_bits(g.h, len(roots), roots.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      imm.ctypes.data_as(C.POINTER(C.c_uint8)), bits.ctypes.data_as(C.POINTER(C.c_uint64)),
                                      words - 1, C.byref(n), None)
    assert st == pkg.fgi.ECAPACITY
    st = lib.fgi_part_last_wave_bits(g.h, bits.ctypes.data_as(C.POINTER(C.c_uint64)), words - 1, C.byref(n))
    assert st == pkg.fgi.ECAPACITY
    # a short cap: FGI_ECAPACITY with the count, the wave has completed, the accessor then returns the list
    short = np.full(len(inv) - 1, 0xABCDABCD, np.uint32)
    st = lib.fgi_part_invalidate_host(g.h, len(roots), roots.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      imm.ctypes.data_as(C.POINTER(C.c_uint8)), short.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      len(short), C.byref(n), None)
    assert st == pkg.fgi.ECAPACITY and n.value == len(inv)
    assert np.all(short == 0xABCDABCD)
    assert np.array_equal(g.part_last_wave_ids(), inv)
    changed = g.dump_states()
    assert not np.array_equal(before[1], changed[1])
    assert np.array_equal(np.flatnonzero(((before[1][:N] & 3) == 1) & ((changed[1][:N] & 3) == 2)), inv)
    g.close()


# ---- 5. across two and three real processes ----------------------------------------------------------------

def _launch(P, tmp_path, *args):
    out = tmp_path / f"p{P}"
    out.mkdir()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={P}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(HERE, "part_host_roots_worker.py"), "--out", str(out), *map(str, args)]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return [dict(np.load(out / f"rank{q}.npz")) for q in range(P)]


@pytest.mark.parametrize("P,labels", [(2, 0), (3, 1)])
def test_host_roots_across_processes(gpu_available, tmp_path, P, labels):
    """The R-MAT 13 scenario's three waves through fgi_part_invalidate_host in P processes (host all-gathers
    over gloo), roots given as numpy arrays; P = 3 is ragged."""
    ranks = _launch(P, tmp_path, "--labels", labels)
    c = RW.RMAT
    n = 1 << c["scale"]
    s, d = O.gen_rmat(c["scale"], c["ef"], c["seed"])
    o = O.Oracle(n)
    o.load_graph(O.version_of(c["seed"], np.arange(n)), None, s, d, O.gen_tags(s, d, c["seed"], 0, c["sseed"]))
    deg = np.bincount(s, minlength=n)
    for w, (k, rseed) in enumerate(RW.WAVES):
        roots = O.gen_roots(k, n, rseed, deg)
        imm = (np.arange(len(roots)) % 5 == 0).astype(np.uint8)
        o.clear_log()
        o.invalidate_slots(roots, imm)
        inv = np.sort(o.inv_log())
        if w == 0:   # (the third wave repeats the first one's roots: little is left for it)
            assert len(inv) > 100 and all(np.any(inv // -(-n // P) == q) for q in range(P))
        for q, res in enumerate(ranks):
            block = int(res["block"][0])
            lo, hi = _range(q, block, n)
            want = inv[(inv >= lo) & (inv < hi)]
            for key in ("call", "ids", "dev"):
                assert np.array_equal(res[f"w{w}_{key}"], want), f"wave {w}, rank {q}: {key} ids differ"
            assert int(res[f"w{w}_n"][0]) == len(want)
            bits = res[f"w{w}_bits"]
            assert len(bits) == (block + 63) // 64
            assert np.array_equal(_bits_to_ids(bits) + lo, want), f"wave {w}, rank {q}: bitmap differs"
            assert np.array_equal(np.sort(res[f"w{w}_export"]), want)
    o.close()


def _bits_to_ids(bits):
    b = np.unpackbits(np.ascontiguousarray(bits, np.uint64).view(np.uint8), bitorder="little")
    return np.flatnonzero(b).astype(np.int64)


# ---- 6. the same addressing as the state view --------------------------------------------------------------

@pytest.mark.parametrize("path", [1, 2])
def test_bitmap_is_addressed_like_the_view(pkg, gpu_available, path):
    """All nodes Consistent, no delays: what one wave takes out of a rank's `consistent` plane is the wave's
    bitmap, word for word."""
    scale, seed, P = 12, 0x5EED0071, 2
    n = 1 << scale
    gs = [pkg.Graph(n // P, n_detached=8, rank=r, world=P, labels=1) for r in range(P)]
    pkg.fgi.part_init_local(gs, n)
    for g in gs:
        g.set_option(pkg.fgi.OPT_PULL_TPB, 1)
        g.set_option(pkg.fgi.OPT_PART_IDS_PATH, path)
        g.part_synth_rmat(scale, 8, seed, 0, 0)
    views = _open(gs, n // P)
    s, _ = O.gen_rmat(scale, 8, seed)
    roots = O.gen_roots(16, n, 0x5EED1071, np.bincount(s, minlength=n))
    before = [v.consistent.copy() for v in views]
    stats = pkg.fgi.part_local_invalidate(gs, roots)
    assert all(x.v_inv > 16 for x in stats)
    for r, (g, view) in enumerate(zip(gs, views)):
        bits, nv = g.part_last_wave_bits()
        assert nv == stats[r].v_inv == int(np.unpackbits(bits.view(np.uint8)).sum())
        assert np.array_equal(before[r] & ~view.consistent, bits), f"rank {r}"
    for g in gs:
        g.close()


# ---- 7. validity -------------------------------------------------------------------------------------------

def _statuses(g):
    lib = g.lib
    n, p = C.c_uint64(), C.c_void_p()
    return [lib.fgi_part_last_wave_ids(g.h, None, 0, C.byref(n)), lib.fgi_part_last_wave_bits(g.h, None, 0, C.byref(n)),
            lib.fgi_part_wave_ids_dev(g.h, C.byref(p), C.byref(n))]


def test_validity(pkg, gpu_available):
    gs, block, n = _chain(pkg, 1, 0)
    for g in gs:
        g.snapshot()
    assert all(_statuses(g) == [pkg.fgi.OK] * 3 for g in gs)
    pkg.fgi.part_local_invalidate(gs, [150])
    for r, g in enumerate(gs):
        _check_rank(pkg, g, r, block, n, np.arange(150, n, dtype=np.uint32), "a wave")
    # a batch ran cascades of its own: its ids left through its out_ids
    ids, _, _ = pkg.fgi.part_local_run_batch(gs, [("invalidate", [100])])
    assert np.array_equal(np.sort(ids), np.arange(100, 150, dtype=np.uint32))
    for g in gs:
        assert _statuses(g) == [pkg.fgi.ENOTSUP] * 3
        with pytest.raises(pkg.FgiError):
            g.part_last_wave_ids()
    # a wave again: valid again, rank by rank, in any order
    pkg.fgi.part_local_invalidate(gs, [70])
    for r in (2, 0, 1):
        _check_rank(pkg, gs[r], r, block, n, np.arange(70, 100, dtype=np.uint32), "a wave after the batch")
    for r, g in enumerate(gs):
        g.restore()
        assert _statuses(g) == [pkg.fgi.OK] * 3
        _check_rank(pkg, g, r, block, n, np.zeros(0, np.uint32), "restored")
    for g in gs:
        g.close()
    single = pkg.Graph(64)
    assert _statuses(single) == [pkg.fgi.ENOTSUP] * 3
    single.close()
