"""CPU-side checks of the replica fan-out per rank of a partition (C-ABI 0.10): the header declares
fgi_part_subscribe, fgi_part_last_wave_fanout, fgi_part_fanout_ids, fgi_part_fanout_detached and
fgi_part_unsubscribe_peer, the library exports them, the binding declares their signatures with the header's
argument counts, and the subscription fixture of test_gpu_part_fanout.py's mixed-state case is not vacuous."""
import ctypes
import functools
import re

import numpy as np
import pytest

from harness import INVALIDATED
from test_gpu_fanout import np_join
from test_gpu_flagged import N, _mixed
from test_state_view_abi import HEADER

NAMES = ["fgi_part_subscribe", "fgi_part_last_wave_fanout", "fgi_part_fanout_ids", "fgi_part_fanout_detached",
         "fgi_part_unsubscribe_peer"]
MIXED_PEERS = 7


def test_header_library_and_binding_agree(pkg):
    names = pkg.fgi.header_symbols(HEADER)
    lib = pkg.load_library()
    for n in NAMES:
        assert n in names, f"{n} is not declared in fgi.h"
        assert hasattr(lib, n), f"libfgi.so does not export {n}"
        assert n in pkg.fgi.SIGNATURES, f"the binding declares no signature for {n}"
    txt = open(HEADER).read()
    assert "#define FGI_SUB_NOT_OWNED 2u" in txt and pkg.fgi.SUB_NOT_OWNED == 2
    for m in ("part_subscribe", "part_last_wave_fanout", "part_fanout_ids", "part_fanout_detached",
              "part_unsubscribe_peer"):
        assert hasattr(pkg.Graph, m), m


def test_signatures_match_the_header(pkg):
    """The argument counts of the binding against the header's declarations (a mismatch would corrupt the
    call, not fail it)."""
    txt = open(HEADER).read()
    for n in NAMES:
        m = re.search(r"fgi_status\s+" + n + r"\s*\(([^;]*)\)\s*;", txt)
        assert m, n
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len([a for a in args.split(",") if a.strip()]) == len(pkg.fgi.SIGNATURES[n]), n


def test_version_is_0_10(pkg):
    lib = pkg.load_library()
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.fgi_version(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) >= (0, 10)


@functools.lru_cache(maxsize=None)
def mixed_subscriptions():
    """The mixed-state case's subscriptions over `_mixed()`'s graph, subscribed once before wave 0: the 6,000
    entries, which of them are stored (an entry on an empty or Invalidated slot completes at once), and per
    wave the stored entries still live when it starts (a mask over the 6,000)."""
    (versions, flags, *_), waves, _ = _mixed()
    rng = np.random.default_rng(4096)
    sh = rng.integers(0, N, 6000).astype(np.uint32)
    sp = rng.integers(0, MIXED_PEERS, 6000).astype(np.uint32)
    sc = (np.uint64(1) << np.uint64(40)) + rng.permutation(6000).astype(np.uint64)   # distinct
    dead = (versions[sh] == 0) | ((flags[sh] & 3) == INVALIDATED)
    live = ~dead
    live_at = []
    for _, _, inv, *_rest in waves:
        live_at.append(live.copy())
        live = live & ~np.isin(sh, inv)
    for a in [sh, sp, sc, dead, live] + live_at:
        a.setflags(write=False)
    return sh, sp, sc, dead, live_at, live


@pytest.mark.parametrize("P", [2, 3, 8])
def test_fixture_is_not_vacuous(P):
    """Conditions on the oracle alone: 5,477 entries are stored and 523 complete at once, and every rank
    delivers at least 9 entries in every one of the three waves (the smallest: rank 5 of 8 in wave 2), so a
    changed generator cannot let a rank pass on nothing."""
    _, waves, _ = _mixed()
    sh, sp, sc, dead, live_at, _ = mixed_subscriptions()
    assert len(np.unique(sc)) == 6000
    assert (int((~dead).sum()), int(dead.sum())) == (5477, 523)
    block = -(-N // P)
    shares = []
    for k, (_, _, inv, *_rest) in enumerate(waves):
        m = live_at[k]
        _, calls, slots = np_join(inv, sh[m], sp[m], sc[m], MIXED_PEERS)
        share = np.bincount(slots // block, minlength=P)
        print(f"P={P} wave {k}: {len(calls)} entries, per rank {share.tolist()}")
        assert share.min() >= 9, (k, share)
        shares.append(share.tolist())
    if P == 2:
        assert shares[0] == [209, 273]
