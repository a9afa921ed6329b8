"""The rules of frontier exploration (include/rmpc.h: rmpc_grid_frontier_device, rmpc_grid_fields_seeded_device,
rmpc_grid_descend_device) as restated in tests/exploration_reference.py, checked on hand-computed cases
and in the kinematic exploration of seeded stores of tests/exploration_cases.py; tests/test_gpu_exploration.py holds the
device against the restatements."""
import ctypes as C
import math

import numpy as np
import pytest

from exploration_cases import KINEMATIC, kinematic, one_seed
from exploration_reference import (BAD_MAP, BAD_SEED, OK, OUTSIDE, TOO_LONG, descend_seeded_ref, field_seeded_ref,
                                   frontier_ref)
from global_planner_reference import S2, descend_ref, field_ref

INF = math.inf


# ---- hand cases on a 4 x 6 map ---------------------------------------------------------------------------------------
H0, W0 = 4, 6


def test_frontier_needs_a_known_free_cell():
    """columns 0 .. 3 seen, 4 and 5 not; (0, 3) lies in the inflation band"""
    misses = np.zeros((H0, W0), dtype=np.int32)
    misses[:, :4] = 2
    hits = np.zeros_like(misses)
    enlarged = np.zeros((H0, W0))
    enlarged[0, 3] = 1.0
    enlarged[2, 5] = 1.0                 # not known: the plan holds unknown_value there, not this
    plan, seed, count = frontier_ref(hits, misses, enlarged, unknown_value=0.9)
    want = np.zeros((H0, W0), dtype=bool)
    want[1:, 3] = True                   # beside column 4; (0, 3) is blocked; column 0 lies at the map's edge: no frontier
    assert count == 3 and np.array_equal(seed == 0.0, want) and np.all(np.isinf(seed[~want]))
    assert np.array_equal(plan[:, :4], enlarged[:, :4]) and np.all(plan[:, 4:] == 0.9)
    # evidence of either kind makes a cell known: a hit alone on (1, 4) takes (1, 3) off the frontier, and (1, 4) itself is
    # known, free on the enlarged grid and beside unknown cells
    hits[1, 4] = 1
    _, seed, count = frontier_ref(hits, misses, enlarged)
    want[1, 3], want[1, 4] = False, True
    assert count == 3 and np.array_equal(seed == 0.0, want)
    # the sum is taken in 64 bits, as rmpc_grid_occupancy_device takes it: two wrapped counters do not cancel to "unknown"
    hits, misses = np.zeros((H0, W0), dtype=np.int32), np.ones((H0, W0), dtype=np.int32)
    hits[1, 1] = misses[1, 1] = -(1 << 31)
    assert frontier_ref(hits, misses, np.zeros((H0, W0)))[2] == 0


def test_frontier_4_against_8_moves():
    misses = np.ones((H0, W0), dtype=np.int32)
    misses[0, 0] = 0
    hits = np.zeros_like(misses)
    z = np.zeros((H0, W0))
    _, seed4, n4 = frontier_ref(hits, misses, z, nmoves=4)
    _, seed8, n8 = frontier_ref(hits, misses, z, nmoves=8)
    assert n4 == 2 and sorted(np.flatnonzero(seed4.ravel() == 0.0)) == [1, W0]
    assert n8 == 3 and sorted(np.flatnonzero(seed8.ravel() == 0.0)) == [1, W0, W0 + 1]


def test_all_unknown_has_no_frontier():
    z = np.zeros((H0, W0), dtype=np.int32)
    plan, seed, count = frontier_ref(z, z, np.zeros((H0, W0)), unknown_value=1.0)
    assert count == 0 and np.all(plan == 1.0) and np.all(np.isinf(seed))
    one = np.ones((H0, W0), dtype=np.int32)
    plan, seed, count = frontier_ref(z, one, np.zeros((H0, W0)))
    assert count == 0 and np.all(plan == 0.0) and np.all(np.isinf(seed))


def _maps():
    rng = np.random.default_rng(5)
    binary = (rng.uniform(size=(12, 15)) < 0.25).astype(float)
    graded = np.where(rng.uniform(size=(12, 15)) < 0.2, 1.0, rng.uniform(0.0, 0.7, (12, 15)))
    return {"binary": binary, "graded": graded}


@pytest.mark.parametrize("kind", ["binary", "graded"])
@pytest.mark.parametrize("movement", [8, 4])
def test_single_seed_equals_the_goal_field(kind, movement):
    data = _maps()[kind]
    for goal in np.flatnonzero(data.ravel() < 0.8)[::17]:
        D, st = field_seeded_ref(data, one_seed(data.shape, [goal]), movement)
        assert st == OK and np.array_equal(D, field_ref(data, int(goal), movement))


@pytest.mark.parametrize("kind", ["binary", "graded"])
def test_two_seeds_equal_the_minimum_of_two_goal_fields(kind):
    data = _maps()[kind]
    free = np.flatnonzero(data.ravel() < 0.8)
    rng = np.random.default_rng(6)
    for _ in range(6):
        a, b = rng.choice(free, 2, replace=False)
        D, st = field_seeded_ref(data, one_seed(data.shape, [a, b]))
        assert st == OK and np.array_equal(D, np.minimum(field_ref(data, int(a)), field_ref(data, int(b))))


def test_a_potential_beside_a_source_is_undercut_and_passed_through():
    data = np.zeros((H0, W0))
    seeds = one_seed(data.shape, [1 * W0 + 2, 1 * W0 + 3], [0.0, 5.0])
    D, st = field_seeded_ref(data, seeds)
    assert st == OK and D[1, 2] == 0.0 and D[1, 3] == 1.0 and D[1, 5] == 3.0 and D[3, 3] == 1.0 + S2
    assert descend_seeded_ref(data, D, seeds, 1 * W0 + 5) == ([11, 10, 9, 8], 4)
    # a potential that nothing undercuts is a source: 0.5 < 1
    seeds = one_seed(data.shape, [1 * W0 + 2, 1 * W0 + 3], [0.0, 0.5])
    D, _ = field_seeded_ref(data, seeds)
    assert D[1, 3] == 0.5 and D[1, 4] == 1.5 and descend_seeded_ref(data, D, seeds, 1 * W0 + 5) == ([11, 10, 9], 3)


def test_seed_rules():
    data = np.zeros((H0, W0))
    data[:, 2] = 1.0                                       # a wall: columns 0, 1 | 3 .. 5
    # a seed on an occupied cell is ignored, whatever it holds; no finite seed left on this side: all +inf, status OK
    seeds = one_seed(data.shape, [2, W0 + 2], [0.0, -1.0])
    D, st = field_seeded_ref(data, seeds)
    assert st == OK and np.all(np.isinf(D))
    seeds[0, 0] = 0.0
    D, st = field_seeded_ref(data, seeds)
    assert st == OK and D[3, 1] == 2.0 + S2 and np.all(np.isinf(D[:, 2:]))
    for bad in (-1e-300, -INF, math.nan):
        seeds[3, 5] = bad
        D, st = field_seeded_ref(data, seeds)
        assert st == BAD_SEED and np.all(np.isinf(D))
    seeds[3, 5] = 0.0
    data[0, 1] = -0.5
    assert field_seeded_ref(data, seeds)[1] == BAD_MAP


def test_descent_starts_and_ends():
    data = np.zeros((H0, W0))
    data[:, 2] = 1.0
    data[3, 5] = 1.0
    data[2, 4] = data[2, 5] = data[3, 4] = 1.0             # (3, 5) is occupied and walled in
    seeds = one_seed(data.shape, [0])
    D, _ = field_seeded_ref(data, seeds)
    # a start on an occupied cell takes one step out, here from (1, 2) in the wall: (1, 1) costs 1 + sqrt 2 and (0, 1)
    # sqrt 2 + 1, a tie, and (1, 1) = move 2 comes before (0, 1) = move 6
    assert np.isinf(D[1, 2]) and D[1, 1] == S2 and D[0, 1] == 1.0
    assert 1.0 + S2 == S2 + 1.0
    assert descend_seeded_ref(data, D, seeds, 1 * W0 + 2) == ([8, 7, 0], 3)
    # a start that is a source
    assert descend_seeded_ref(data, D, seeds, 0) == ([0], 1)
    # walled in: an occupied start without a finite neighbour, a free start that no source reaches
    assert descend_seeded_ref(data, D, seeds, 3 * W0 + 5) == ([], 0)
    assert np.isinf(D[0, 4]) and descend_seeded_ref(data, D, seeds, 0 * W0 + 4) == ([], 0)
    # outside, and a route longer than max_len
    assert descend_seeded_ref(data, D, seeds, -1)[1] == OUTSIDE and descend_seeded_ref(data, D, seeds, H0 * W0)[1] == OUTSIDE
    assert descend_seeded_ref(data, D, seeds, 3 * W0, max_len=2) == ([18, 12], TOO_LONG)
    assert descend_seeded_ref(data, D, seeds, 3 * W0, max_len=4) == ([18, 12, 6, 0], 4)
    # on a single seed the walk is the goal descent
    assert descend_seeded_ref(data, D, seeds, 3 * W0 + 1)[0] == descend_ref(data, field_ref(data, 0), 3 * W0 + 1, 0)


# ---- kinematic exploration: robots that move one cell per step along the descent ---------------------------------------
@pytest.mark.parametrize("seed,B,free", KINEMATIC)
def test_kinematic_exploration_ends_sees_every_free_cell_and_stays_clear(seed, B, free):
    """The rules end on their own: no frontier is left within 1500 steps (the first re-plan without one came at step
    105, 100, 50 and 125 here), no free cell is unseen then, and no robot ever stands on a cell of the truly enlarged
    map.  The last of the three rests on the order of the control step: a route is planned from what the scans have
    shown, and the cells a few steps ahead of a robot are the ones its own 64 rays cover without gaps.  With the
    re-plan before the follower's step (five moves per route instead of four) 1, 0, 2 and 3 robot-steps of these four
    runs end on such a cell, each the fifth move of a route whose last cell lies beside a shelf cell not yet seen."""
    r = kinematic(seed, B)
    assert r["ended"] is not None and r["ended"] < 1500, r
    assert r["free"] == free and r["unseen"] == 0, r
    assert r["on_enlarged"] == 0, r


def test_corner_starts_are_clear_and_packed():
    from robot_mpcs_amd.global_planner import shelf_map
    from robot_mpcs_amd.utils.exploration import corner_starts
    raw = shelf_map(41, 41, seed=0, aisle=6, shelf=2, gap=5)
    c = corner_starts(raw, 64)
    assert c.dtype == np.int32 and len(set(c.tolist())) == 64 and c[0] == 3 * 41 + 3
    for cell in c:
        r, col = divmod(int(cell), 41)
        assert not (raw[r - 2:r + 3, col - 2:col + 3] > 0.5).any()
    d2 = (c // 41) ** 2 + (c % 41) ** 2
    assert np.all(np.diff(d2) >= 0) and np.array_equal(c[:8], corner_starts(raw, 8))
    with pytest.raises(ValueError):
        corner_starts(raw, 41 * 41)


# ---- the refusals of the three entries, before any HIP call --------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return _lib


def test_new_entries_and_status_code_are_exported(lib):
    assert {"rmpc_grid_frontier_device", "rmpc_grid_fields_seeded_device", "rmpc_grid_descend_device"} <= set(lib.EXPORTED_SYMBOLS)
    assert lib.GRID_BAD_SEED == BAD_SEED == -7
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rmpc.h")).read()
    assert "#define RMPC_GRID_BAD_SEED (-7)" in hdr


def test_refusals(lib):
    """Each refusal returns -1 with the entry's own message, never the HIP runtime's: host-side fake pointers are never
    dereferenced, and a call that passed validation would report a HIP error on a machine without a device."""
    L = lib.load_library()
    P = C.c_void_p(0x1000)
    nan, inf = math.nan, math.inf

    def frontier(H=41, W=41, hits=P, misses=P, enl=P, occ=0.8, nmoves=4, unk=1.0, plan=P, seed=P, count=P):
        rc = L.rmpc_grid_frontier_device(H, W, hits, misses, enl, occ, nmoves, unk, plan, seed, count, None)
        return rc, L.rmpc_last_error().decode()

    cases = [(dict(hits=None), "null argument"), (dict(misses=None), "null argument"), (dict(enl=None), "null argument"),
             (dict(plan=None), "null argument"), (dict(seed=None), "null argument"), (dict(count=None), "null argument"),
             (dict(H=0), "need H, W >= 1"), (dict(W=-3), "need H, W >= 1"), (dict(H=129, W=128), "RMPC_GRID_MAX_CELLS"),
             (dict(H=1 << 16, W=1 << 16), "RMPC_GRID_MAX_CELLS"), (dict(nmoves=0), "nmoves must be 4 or 8"),
             (dict(nmoves=6), "nmoves must be 4 or 8"), (dict(occ=nan), "must be finite"), (dict(occ=inf), "must be finite"),
             (dict(unk=nan), "must be finite"), (dict(unk=-inf), "must be finite")]
    for kw, want in cases:
        rc, msg = frontier(**kw)
        assert rc == -1 and want in msg and "hip" not in msg.lower(), (kw, msg)

    def seeded(H=41, W=41, grid=P, G=1, seeds=P, mv=8, occ=0.8, f=3.0, fields=P, status=P, sweeps=None):
        rc = L.rmpc_grid_fields_seeded_device(H, W, grid, G, seeds, mv, occ, f, fields, status, sweeps, None)
        return rc, L.rmpc_last_error().decode()

    cases = [(dict(grid=None), "null argument"), (dict(seeds=None), "null argument"), (dict(fields=None), "null argument"),
             (dict(status=None), "null argument"), (dict(H=0), "need H, W >= 1"), (dict(W=0), "need H, W >= 1"),
             (dict(mv=5), "movement must be 4 or 8"), (dict(H=129, W=128), "RMPC_GRID_MAX_CELLS"), (dict(G=0), "1 <= G"),
             (dict(G=1 << 21), "INT_MAX"), (dict(f=-1.0), "cost_factor"), (dict(f=nan), "cost_factor"),
             (dict(f=inf), "cost_factor")]
    for kw, want in cases:
        rc, msg = seeded(**kw)
        assert rc == -1 and want in msg and "hip" not in msg.lower(), (kw, msg)

    def descend(H=41, W=41, grid=P, G=1, fields=P, seeds=P, B=4, start=P, fi=P, mv=8, occ=0.8, f=3.0, max_len=10, path=P,
                ln=P):
        rc = L.rmpc_grid_descend_device(H, W, grid, G, fields, seeds, B, start, fi, mv, occ, f, max_len, path, ln, None)
        return rc, L.rmpc_last_error().decode()

    cases = [(dict(grid=None), "null argument"), (dict(fields=None), "null argument"), (dict(seeds=None), "null argument"),
             (dict(start=None), "null argument"), (dict(fi=None), "null argument"), (dict(path=None), "null argument"),
             (dict(ln=None), "null argument"), (dict(H=0), "need H, W >= 1"), (dict(mv=3), "movement must be 4 or 8"),
             (dict(G=0), "1 <= G"), (dict(H=1 << 12, W=1 << 12, G=1 << 10), "INT_MAX"), (dict(B=0), "B, max_len >= 1"),
             (dict(max_len=0), "B, max_len >= 1"), (dict(B=1 << 20, max_len=1 << 12), "INT_MAX"),
             (dict(f=-1.0), "cost_factor"), (dict(f=nan), "cost_factor"), (dict(f=inf), "cost_factor")]
    for kw, want in cases:
        rc, msg = descend(**kw)
        assert rc == -1 and want in msg and "hip" not in msg.lower(), (kw, msg)
