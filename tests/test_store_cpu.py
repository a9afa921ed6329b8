"""robot_mpcs_amd/store.py without a GPU: the store's record, ``clear_cells`` and ``box_distance`` against brute force; and
every refusal of the grid entries of rmpc_world.hip that a host check makes before the first HIP call, with its full
text."""
import ctypes as C
import math

import numpy as np
import pytest

NAN, INF = math.nan, math.inf


# ---- the store ---------------------------------------------------------------------------------------------------------
def test_store_record_holds_the_examples_constants():
    """the values examples/fleet_store_lidar.py defined as module constants before they moved"""
    from robot_mpcs_amd.store import STORE
    assert STORE._asdict() == dict(H=41, W=41, cell=0.45, x0=-9.0, y0=-9.0, aisle=6, shelf=2, gap=5, size_robot=0.45,
                                   r_body=0.6, ee_offset=0.4, clear_cells=2)


def dilation_ref(raw, k):
    """free cells with no occupied cell (the outside of the map counts as occupied) within Chebyshev distance k, cell by
    cell"""
    H, W = raw.shape
    out = np.zeros((H, W), dtype=bool)
    for r in range(H):
        for c in range(W):
            out[r, c] = all(0 <= r + dr < H and 0 <= c + dc < W and raw[r + dr, c + dc] <= 0.5
                            for dr in range(-k, k + 1) for dc in range(-k, k + 1))
    return out


@pytest.mark.parametrize("H,W,k", [(23, 37, 2), (37, 23, 1), (5, 7, 0), (41, 41, 2)])
def test_clear_cells_is_the_chebyshev_dilation_on_any_shape(H, W, k):
    from robot_mpcs_amd.global_planner import shelf_map
    from robot_mpcs_amd.store import clear_cells
    raw = shelf_map(H, W, seed=1, aisle=5, shelf=2, gap=2)
    got = clear_cells(raw, k)
    assert got.shape == (H, W) and got.dtype == bool
    assert np.array_equal(got, dilation_ref(raw, k))
    assert k == 0 or 0 < got.sum() < (raw <= 0.5).sum()


def test_clear_cells_of_the_store_is_the_mask_of_corner_starts():
    from robot_mpcs_amd.store import STORE, clear_cells, store_map
    from robot_mpcs_amd.utils.exploration import corner_starts
    raw = store_map(0)
    mask = clear_cells(raw, 2)
    assert np.array_equal(mask, dilation_ref(raw, 2))
    n = int(mask.sum())
    assert np.array_equal(np.sort(corner_starts(raw, n, STORE.clear_cells)), np.flatnonzero(mask.ravel()))
    with pytest.raises(ValueError):
        corner_starts(raw, n + 1, STORE.clear_cells)


def test_box_distance_against_a_loop_over_points():
    import torch
    from robot_mpcs_amd.store import box_distance
    rng = np.random.default_rng(5)
    boxes = np.array([[0.0, 0.0, 2.0, 1.0], [3.0, 2.0, 0.5, 4.0], [-4.0, 1.0, 1.0, 1.0]])
    p = np.concatenate([rng.uniform(-6.0, 6.0, (200, 2)),
                        [[0.25, -0.25],      # inside box 0
                         [1.0, 0.2],         # on an edge of box 0
                         [1.0, 0.5],         # on a corner of box 0
                         [3.0, 5.0]]])       # 1 m off an edge of box 1
    want = np.empty(len(p))
    for i, (x, y) in enumerate(p):
        d = [math.hypot(max(abs(x - cx) - 0.5 * lx, 0.0), max(abs(y - cy) - 0.5 * ly, 0.0)) for cx, cy, lx, ly in boxes]
        want[i] = min(d)
    got = box_distance(torch.from_numpy(p), torch.from_numpy(boxes)).numpy()
    assert got.shape == (len(p),)
    assert np.allclose(got, want, rtol=0.0, atol=1e-15)
    assert got[200] == 0.0 and got[201] == 0.0 and got[202] == 0.0 and got[203] == 1.0
    assert (got[:200] > 0.0).sum() > 150


# ---- the refusals of the grid entries ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return _lib


P = 0x1000      # a host-side fake pointer: a refusal never dereferences it
NULL = "null argument"
GRID_HW = "grid: need H, W >= 1"
GRID_MV = "grid: movement must be 4 or 8"
MAX_LONG = " map exceeds RMPC_GRID_MAX_CELLS = 16384 cells (one field must fit in the LDS of a workgroup)"
MAX_SHORT = ": need H, W >= 1 and H*W <= RMPC_GRID_MAX_CELLS = 16384"
G_HW = ": need 1 <= G and G*H*W <= INT_MAX"
B_LEN = ": need B, max_len >= 1 and B*max_len <= INT_MAX"
COST = ": cost_factor must be finite and >= 0"

# entry -> (the symbols that share the body, their message prefixes, the argument list in the ABI's order with defaults)
ENTRIES = {
    "inflate": (["rmpc_grid_inflate_device"], ["grid inflate"],
                dict(H=41, W=41, cell=0.45, size_robot=0.45, threshold=0.29, grid=P, out=P)),
    "fields": (["rmpc_grid_fields_device", "rmpc_grid_fields_seeded_device"], ["grid fields", "grid fields"],
               dict(H=41, W=41, grid=P, G=1, src=P, mv=8, occ=0.8, f=3.0, fields=P, status=P, sweeps=None)),
    "paths": (["rmpc_grid_paths_device", "rmpc_grid_descend_device"], ["grid paths", "grid descend"],
              dict(H=41, W=41, grid=P, G=1, fields=P, ends=P, B=4, start=P, index=P, mv=8, occ=0.8, f=3.0, max_len=10,
                   path=P, ln=P)),
    "cells": (["rmpc_grid_cells_device"], ["grid cells"],
              dict(B=4, pos=P, stride=8, H=41, W=41, x0=-9.0, y0=-9.0, cell=0.45, cells=P)),
    "follow_path": (["rmpc_follow_path_device"], ["follow path"],
                    dict(B=4, path=P, ln=P, max_len=10, idx=P, pos=P, stride=8, W=41, x0=-9.0, y0=-9.0, cell=0.45,
                         threshold=1.3, goal=P)),
    "occupancy": (["rmpc_grid_occupancy_device"], ["grid occupancy"],
                  dict(H=41, W=41, hits=P, misses=P, w_hit=3, w_miss=1, forget=0, free=0.0, occ=1.0, unk=0.5, grid=P)),
    "frontier": (["rmpc_grid_frontier_device"], ["grid frontier"],
                 dict(H=41, W=41, hits=P, misses=P, enl=P, occ=0.8, nmoves=4, unk=1.0, plan=P, seed=P, count=P)),
}
MARK = dict(rays=64, origins=P, points=P, ranges=P, range=10.0, hit_depth=1e-6, H=41, W=41, x0=-9.0, y0=-9.0, cell=0.45,
            hits=P, misses=P, skipped=None)

# (entry, the bad arguments, the whole message; "{p}" = the entry's prefix): one call per host check that fails before the
# first HIP call, in the order of the checks
REFUSALS = [
    ("inflate", dict(grid=None), NULL), ("inflate", dict(out=None), NULL),
    ("inflate", dict(H=0), GRID_HW), ("inflate", dict(H=1 << 16, W=1 << 16), GRID_HW),
    ("fields", dict(grid=None), NULL), ("fields", dict(src=None), NULL), ("fields", dict(fields=None), NULL),
    ("fields", dict(status=None), NULL),
    ("fields", dict(W=0), GRID_HW), ("fields", dict(mv=5), GRID_MV),
    ("fields", dict(H=129, W=128), "{p}: 129x128" + MAX_LONG),
    ("fields", dict(G=0), "{p}" + G_HW), ("fields", dict(G=1 << 21), "{p}" + G_HW),
    ("fields", dict(f=-1.0), "{p}" + COST), ("fields", dict(f=NAN), "{p}" + COST), ("fields", dict(f=INF), "{p}" + COST),
    ("fields", dict(H=129, W=128, G=0, f=NAN), "{p}: 129x128" + MAX_LONG), ("fields", dict(G=0, f=NAN), "{p}" + G_HW),
    ("paths", dict(grid=None), NULL), ("paths", dict(fields=None), NULL), ("paths", dict(ends=None), NULL),
    ("paths", dict(start=None), NULL), ("paths", dict(index=None), NULL), ("paths", dict(path=None), NULL),
    ("paths", dict(ln=None), NULL),
    ("paths", dict(H=-1), GRID_HW), ("paths", dict(mv=3), GRID_MV),
    ("paths", dict(G=0), "{p}" + G_HW), ("paths", dict(H=1 << 12, W=1 << 12, G=1 << 10), "{p}" + G_HW),
    ("paths", dict(B=0), "{p}" + B_LEN), ("paths", dict(max_len=0), "{p}" + B_LEN),
    ("paths", dict(B=1 << 20, max_len=1 << 12), "{p}" + B_LEN),
    ("paths", dict(f=-1.0), "{p}" + COST), ("paths", dict(f=NAN), "{p}" + COST), ("paths", dict(f=INF), "{p}" + COST),
    ("paths", dict(G=0, B=0, f=NAN), "{p}" + G_HW), ("paths", dict(B=0, f=NAN), "{p}" + B_LEN),
    ("cells", dict(pos=None), NULL), ("cells", dict(cells=None), NULL),
    ("cells", dict(B=0), "{p}: need B >= 1, stride >= 2, B*stride <= INT_MAX"),
    ("cells", dict(stride=1), "{p}: need B >= 1, stride >= 2, B*stride <= INT_MAX"),
    ("cells", dict(B=1 << 20, stride=1 << 12), "{p}: need B >= 1, stride >= 2, B*stride <= INT_MAX"),
    ("cells", dict(H=0), GRID_HW),
    ("follow_path", dict(path=None), NULL), ("follow_path", dict(goal=None), NULL),
    ("follow_path", dict(B=0), "{p}" + B_LEN), ("follow_path", dict(max_len=0), "{p}" + B_LEN),
    ("follow_path", dict(B=1 << 20, max_len=1 << 12), "{p}" + B_LEN),
    ("follow_path", dict(stride=1), "{p}: need stride >= 2, W >= 1"), ("follow_path", dict(W=0), "{p}: need stride >= 2, W >= 1"),
    ("mark", dict(m=None), NULL), ("mark", dict(struct_size=8), "rmpc_grid_mark.struct_size mismatch"),
    ("mark", dict(B=0), "{p}: need B >= 1 and rays >= 1"), ("mark", dict(rays=0), "{p}: need B >= 1 and rays >= 1"),
    ("mark", dict(B=1 << 20, rays=1 << 10), "{p}: B*rays*3 must not exceed INT_MAX"),
    ("mark", dict(H=0), "{p}" + MAX_SHORT), ("mark", dict(H=129, W=128), "{p}" + MAX_SHORT),
    ("mark", dict(H=1 << 16, W=1 << 16), "{p}" + MAX_SHORT),
    ("mark", dict(cell=0.0), "{p}: cell and range must be positive and finite"),
    ("mark", dict(range=INF), "{p}: cell and range must be positive and finite"),
    ("mark", dict(hit_depth=-1.0), "{p}: hit_depth must be finite and >= 0"),
    ("mark", dict(x0=NAN), "{p}: x0, y0 must be finite"),
    ("mark", dict(origins=None), NULL), ("mark", dict(misses=None), NULL),
    ("mark", dict(range=1e9, cell=1.0), "{p}: (range + hit_depth) / cell must not exceed 2^29 cells"),
    ("occupancy", dict(hits=None), NULL), ("occupancy", dict(grid=None), NULL),
    ("occupancy", dict(W=0), "{p}" + MAX_SHORT), ("occupancy", dict(H=129, W=128), "{p}" + MAX_SHORT),
    ("occupancy", dict(w_hit=0), "{p}: need w_hit, w_miss >= 1"), ("occupancy", dict(forget=32), "{p}: forget must lie in [0, 31]"),
    ("occupancy", dict(unk=NAN), "{p}: the three values must be finite"),
    ("frontier", dict(enl=None), NULL), ("frontier", dict(count=None), NULL),
    ("frontier", dict(H=0), "{p}" + MAX_SHORT), ("frontier", dict(H=129, W=128), "{p}" + MAX_SHORT),
    ("frontier", dict(nmoves=6), "{p}: nmoves must be 4 or 8"),
    ("frontier", dict(occ=INF), "{p}: occ_threshold and unknown_value must be finite"),
]


def call_mark(lib, L, bad):
    bad = dict(bad)
    B = bad.pop("B", 4)
    if "m" in bad:
        return L.rmpc_grid_mark_device(B, None, None)
    a = lib.GridMarkArgs()
    a.struct_size = bad.pop("struct_size", C.sizeof(lib.GridMarkArgs))
    for k, v in dict(MARK, **bad).items():
        setattr(a, k, v)
    return L.rmpc_grid_mark_device(B, C.byref(a), None)


@pytest.mark.parametrize("entry,bad,want", REFUSALS, ids=["%s-%s" % (e, ",".join(b)) for e, b, _ in REFUSALS])
def test_grid_entry_refusal_text(lib, entry, bad, want):
    """Each refusal returns -1 with exactly the message the entry has always given -- the first failing check's -- and
    the entries that share a body (fields / fields_seeded, paths / descend) give the same one up to the prefix."""
    L = lib.load_library()
    if entry == "mark":
        assert call_mark(lib, L, bad) == -1
        assert L.rmpc_last_error().decode() == want.format(p="grid mark")
        return
    symbols, prefixes, args = ENTRIES[entry]
    assert set(bad) <= set(args)
    for sym, p in zip(symbols, prefixes):
        assert getattr(L, sym)(*dict(args, **bad).values(), None) == -1, sym
        assert L.rmpc_last_error().decode() == want.format(p=p), sym
