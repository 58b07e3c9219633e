"""CPU-side checks of the partitioned state view's boundary (C-ABI 0.7): the header declares
fgi_part_state_view_open and fgi_part_view_is_consistent, the library exports them, the binding declares
their signatures, and the exported helper routes a global slot to its rank's view."""
import ctypes

import numpy as np

from test_gpu_state_view import PLANES, planes_from_flags
from test_state_view_abi import CANONICAL, HEADER

NAMES = ["fgi_part_state_view_open", "fgi_part_view_is_consistent"]


def test_header_library_and_binding_agree(pkg):
    names = pkg.fgi.header_symbols(HEADER)
    lib = pkg.load_library()
    for n in NAMES:
        assert n in names, f"{n} is not declared in fgi.h"
        assert hasattr(lib, n), f"libfgi.so does not export {n}"
        assert n in pkg.fgi.SIGNATURES, f"the binding declares no signature for {n}"
    assert "#define FGI_OPT_PART_VIEW_PATH 18" in open(HEADER).read() and pkg.fgi.OPT_PART_VIEW_PATH == 18
    assert hasattr(pkg.Graph, "part_open_state_view") and hasattr(pkg.fgi, "part_view_is_consistent")


def test_version_is_0_7(pkg):
    lib = pkg.load_library()
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.fgi_version(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) >= (0, 7)


def test_exported_helper_routes_a_slot_to_its_rank(pkg):
    """Three hand-built views of 70 handles each in ordinary memory (no device): global slot s is handle
    s % 70 of view s // 70; slots past p * block are not Consistent."""
    lib = pkg.load_library()
    p, block = 3, 70
    flags = np.array((CANONICAL + [0]) * 15, np.uint32)[:p * block]
    # rotate the pattern per rank so that the same handle differs between the views
    flags = np.concatenate([np.roll(flags[r * block:(r + 1) * block], r) for r in range(p)])
    versions = np.where(np.arange(p * block) % 15 == 14, 0, 1 + np.arange(p * block)).astype(np.uint64)
    want = (versions != 0) & ((flags & 3) == 1)
    keep = []
    views = (pkg.fgi.StateViewStruct * p)()
    for r in range(p):
        planes = planes_from_flags(versions[r * block:(r + 1) * block], flags[r * block:(r + 1) * block])
        keep.append(planes)
        views[r].struct_size, views[r].n_handles, views[r].words = ctypes.sizeof(views[r]), block, 2
        for k in PLANES:
            setattr(views[r], k, planes[k].ctypes.data)
    # the slots at the ranks' edges are of both kinds, so a helper that routed them wrongly would show
    edges = [0, 69, 70, 139, 140, 209]
    assert len({bool(want[s]) for s in edges}) == 2
    for s in range(p * block):
        assert lib.fgi_part_view_is_consistent(views, p, block, s) == int(want[s]), s
    for s in edges:
        assert lib.fgi_part_view_is_consistent(views, p, block, s) == int(want[s]), s
    for s in (p * block, p * block + 1, 0xFFFFFFFF):
        assert lib.fgi_part_view_is_consistent(views, p, block, s) == 0, s
    assert lib.fgi_part_view_is_consistent(views, p, 0, 5) == 0   # no block: no slot
