"""Cost-to-go fields on large maps (include/rmpc_grid_large.h), what needs no GPU: the second header and
its tables, every refusal of the two entries by whole message, and the work-list rule restated in numpy
(tests/grid_large_reference.py) against the heap Dijkstras of the recursion."""
import math
import os
import re

import numpy as np
import pytest

from exploration_reference import field_seeded_ref
from global_planner_reference import field_ref
from grid_large_reference import ORDERS, serpentine, tiled_field_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = math.inf, math.nan
SYMBOLS = ["rmpc_grid_fields_large_device", "rmpc_grid_fields_seeded_large_device"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return _lib


# ---- the header and the binding ---------------------------------------------------------------------------------------
def test_large_symbols_are_declared_by_the_new_header_and_exported(lib):
    from robot_mpcs_amd import _abi
    assert lib.GRID_LARGE_SYMBOLS == SYMBOLS == list(_abi.large_prototypes)
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rmpc_grid_large.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(rmpc_\w+)\s*\(", code))) == sorted(SYMBOLS)
    L = lib.load_library()
    for sym in SYMBOLS:
        fn = getattr(L, sym)
        assert (fn.restype, list(fn.argtypes)) == (_abi.large_prototypes[sym][0], _abi.large_prototypes[sym][1])
    # the same argument lists as the entries of rmpc.h they stand beside
    assert _abi.large_prototypes[SYMBOLS[0]] == _abi.prototypes["rmpc_grid_fields_device"]
    assert _abi.large_prototypes[SYMBOLS[1]] == _abi.prototypes["rmpc_grid_fields_seeded_device"]


def test_rmpc_h_declares_what_it_declared(lib):
    from robot_mpcs_amd import _abi
    assert len(lib.EXPORTED_SYMBOLS) == 65
    assert not set(SYMBOLS) & set(lib.EXPORTED_SYMBOLS) and not set(SYMBOLS) & set(_abi.prototypes)
    assert not set(_abi.large_constants) & set(_abi.constants)


def test_large_constants(lib):
    assert lib.GRID_LARGE_MAX_CELLS == 2048 * 2048 and lib.GRID_LARGE_MAX_SIDE == 8192
    assert lib.GRID_TILE >= 4 and lib.GRID_LARGE_MAX_CELLS > lib.GRID_MAX_CELLS
    with open(os.path.join(ROOT, "robot_mpcs_amd", "csrc", "sources.txt")) as f:
        listed = f.read().split()
    assert "include/rmpc_grid_large.h" in listed and "robot_mpcs_amd/csrc/rmpc_grid_large.hpp" in listed


# ---- the refusals: host checks that fail before the first HIP call, in the order of the checks ------------------------
P = 0x1000      # a host-side fake pointer: a refusal never dereferences it
ARGS = dict(H=300, W=300, grid=P, G=1, src=P, mv=8, occ=0.8, f=3.0, fields=P, status=P, visits=None)
WHO = "grid fields large"
NULL = "null argument"
HW = WHO + ": need H, W >= 1"
MV = WHO + ": movement must be 4 or 8"
SIDE = " map has a side above RMPC_GRID_LARGE_MAX_SIDE = 8192"
CELLS = " map exceeds RMPC_GRID_LARGE_MAX_CELLS = 4194304 cells"
G_HW = WHO + ": need 1 <= G and G*H*W <= INT_MAX"
COST = WHO + ": cost_factor must be finite and >= 0"
I_MAX, I_MIN = 2 ** 31 - 1, -2 ** 31
REFUSALS = [
    (dict(grid=None), NULL), (dict(src=None), NULL), (dict(fields=None), NULL), (dict(status=None), NULL),
    (dict(H=0), HW), (dict(W=0), HW), (dict(H=-1), HW), (dict(H=I_MIN), HW), (dict(W=I_MIN), HW),
    (dict(mv=5), MV), (dict(mv=0), MV), (dict(mv=I_MAX), MV), (dict(mv=I_MIN), MV),
    (dict(H=8193, W=1), WHO + ": 8193x1" + SIDE), (dict(H=1, W=8193), WHO + ": 1x8193" + SIDE),
    (dict(H=I_MAX, W=I_MAX), WHO + ": 2147483647x2147483647" + SIDE),
    (dict(H=2049, W=2048), WHO + ": 2049x2048" + CELLS), (dict(H=8192, W=513), WHO + ": 8192x513" + CELLS),
    (dict(H=8192, W=8192), WHO + ": 8192x8192" + CELLS),
    (dict(G=0), G_HW), (dict(G=-1), G_HW), (dict(G=I_MIN), G_HW), (dict(G=I_MAX), G_HW),
    (dict(H=2048, W=2048, G=512), G_HW),
    (dict(f=-1.0), COST), (dict(f=NAN), COST), (dict(f=INF), COST), (dict(f=-INF), COST),
    # the first failing check speaks
    (dict(grid=None, H=0), NULL), (dict(H=0, mv=5), HW), (dict(mv=5, H=8193), MV),
    (dict(H=8193, W=8193, G=0), WHO + ": 8193x8193" + SIDE), (dict(H=2049, W=2048, G=0, f=NAN), WHO + ": 2049x2048" + CELLS),
    (dict(G=0, f=NAN), G_HW),
]


@pytest.mark.parametrize("bad,want", REFUSALS, ids=[",".join("%s=%s" % kv for kv in b.items()) for b, _ in REFUSALS])
def test_large_entry_refusal_text(lib, bad, want):
    L = lib.load_library()
    assert set(bad) <= set(ARGS)
    for sym in SYMBOLS:
        assert getattr(L, sym)(*dict(ARGS, **bad).values(), None) == -1, sym
        assert L.rmpc_last_error().decode() == want, sym


def test_the_old_entries_keep_their_cap_and_wording(lib):
    L = lib.load_library()
    for sym in ("rmpc_grid_fields_device", "rmpc_grid_fields_seeded_device"):
        assert getattr(L, sym)(*dict(ARGS, H=129, W=128).values(), None) == -1
        assert L.rmpc_last_error().decode() == ("grid fields: 129x128 map exceeds RMPC_GRID_MAX_CELLS = 16384 cells "
                                                 "(one field must fit in the LDS of a workgroup)")


# ---- the work-list rule against the Dijkstras -------------------------------------------------------------------------
def _tile(lib):
    from robot_mpcs_amd import _abi
    return _abi.large_constants["RMPC_GRID_TILE"]


def _maps():
    """(name, data, goal cell) of the goal cases"""
    from robot_mpcs_amd.global_planner import shelf_map
    from robot_mpcs_amd import _abi
    T = _abi.large_constants["RMPC_GRID_TILE"]
    rng = np.random.default_rng(22)
    out = [("store", shelf_map(41, 41), 42)]
    for H, W in ((129, 128), (150, 131)):
        binary = (rng.uniform(size=(H, W)) < 0.25).astype(float)
        graded = np.where(rng.uniform(size=(H, W)) < 0.2, 1.0, rng.uniform(0.0, 0.7, size=(H, W)))
        for name, d in (("binary", binary), ("graded", graded)):
            free = np.flatnonzero(d.ravel() < 0.8)
            out.append(("%s%dx%d" % (name, H, W), d, int(free[len(free) // 3])))
    out.append(("serpentine", serpentine(2 * T + 3, 2 * T + 5), 0))
    out.append(("row", np.where(np.arange(3 * T + 2) == 2 * T + 1, 1.0, 0.3)[None, :], 5))
    out.append(("column", np.where(np.arange(3 * T + 2) == T, 1.0, 0.3)[:, None], 3 * T))
    walled = np.zeros((2 * T + 1, T + 3))
    walled[T - 2:T + 1, 3:6] = 1.0
    walled[T - 1, 4] = 0.0
    out.append(("walled-in goal", walled, (T - 1) * (T + 3) + 4))
    return out


MAPS = _maps()
REFS = {}


def _ref(name, data, goal, movement):
    """one Dijkstra per case, shared by the tile sizes and orders"""
    if (name, movement) not in REFS:
        REFS[name, movement] = field_ref(data, goal, movement)
        REFS[name, movement].setflags(write=False)
    return REFS[name, movement]


@pytest.mark.parametrize("movement", [8, 4])
@pytest.mark.parametrize("case", range(len(MAPS)), ids=[m[0] for m in MAPS])
def test_tiled_rule_reaches_the_dijkstra_field(lib, case, movement):
    name, data, goal = MAPS[case]
    ref = _ref(name, data, goal, movement)
    for tile in (_tile(lib), 4, 7):
        for order in ORDERS:
            D, visits = tiled_field_ref(data, goal, tile, movement, order)
            assert np.array_equal(D, ref), (name, tile, order)
            assert visits >= 1


def test_walled_in_goal_stays_alone():
    name, data, goal = MAPS[-1]
    D, visits = tiled_field_ref(data, goal, 7, 8, "zigzag")
    assert D.ravel()[goal] == 0.0 and np.isinf(np.delete(D.ravel(), goal)).all()


def test_a_source_on_a_tile_edge_wakes_the_tile_beside_it():
    """The goal's neighbours inside its own tile are occupied, the way out leads straight into the next tile: nothing of
    the goal's tile is ever lowered, so the source itself has to count as a lowered cell."""
    data = np.zeros((8, 8))
    data[3, 2] = data[2, 3] = data[2, 2] = 1.0        # goal (3, 3), the last cell of tile (0, 0) of 4 x 4
    for movement in (4, 8):
        ref = field_ref(data, 3 * 8 + 3, movement)
        assert np.isfinite(ref[5, 5])
        for order in ORDERS:
            D, visits = tiled_field_ref(data, 3 * 8 + 3, 4, movement, order)
            assert np.array_equal(D, ref) and visits >= 4


@pytest.mark.parametrize("movement", [8, 4])
def test_tiled_rule_on_seeded_grids_with_potentials(lib, movement):
    rng = np.random.default_rng(5 + movement)
    for H, W, n in ((150, 131, 60), (40, 37, 9)):
        data = np.where(rng.uniform(size=(H, W)) < 0.2, 1.0, rng.uniform(0.0, 0.7, size=(H, W)))
        seeds = np.full((H, W), INF)
        seeds.ravel()[rng.choice(H * W, n, replace=False)] = rng.uniform(0.0, 20.0, n)     # some on occupied cells
        ref, status = field_seeded_ref(data, seeds, movement)
        assert status == 0
        for tile in ((_tile(lib),) if H > 40 else (4, 7)):
            for order in ORDERS:
                D, visits = tiled_field_ref(data, seeds, tile, movement, order)
                assert np.array_equal(D, ref), (H, tile, order)
    # no finite seed: nothing to visit
    D, visits = tiled_field_ref(data, np.full((H, W), INF), 7, movement, "zigzag")
    assert np.isinf(D).all() and visits == 0


def test_visit_counts_of_both_orders(lib, record_property):
    """The counts the choice of the order rests on, on smaller editions of the two maps named there so
    that the test stays quick: ascending / descending passes take fewer visits than least key first."""
    from robot_mpcs_amd.global_planner import shelf_map
    T = _tile(lib)
    counts = {}
    for name, data, goal in (("shelf_map(192, 192)", shelf_map(192, 192), 193), ("serpentine(131, 133)", MAPS[5][1], 0)):
        for order in ORDERS:
            _, counts[name, order] = tiled_field_ref(data, goal, T, 8, order)
            record_property("%s %s" % (name, order), counts[name, order])
    print("tile visits, tile %d, 8 moves: %s" % (T, {"%s, %s" % k: v for k, v in counts.items()}))
    for name in ("shelf_map(192, 192)", "serpentine(131, 133)"):
        assert counts[name, "zigzag"] <= counts[name, "least"]
