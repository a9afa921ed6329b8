"""The rules of coordinated exploration (include/rmpc.h: rmpc_grid_targets_device, rmpc_grid_route_costs_device,
rmpc_assign_greedy_device) as restated in tests/assignment_reference.py, checked on hand-computed cases
and in the kinematic exploration of tests/exploration_cases.py with one target per tile; tests/test_gpu_assignment.py
holds the device against the restatements."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from assignment_cases import random_costs
from assignment_reference import greedy_ref, greedy_sorted_ref, route_costs_ref, takeable_of, targets_ref, tiles_of
from exploration_cases import KINEMATIC, kinematic, one_seed
from exploration_reference import OK, descend_seeded_ref, field_seeded_ref, frontier_ref
from global_planner_reference import S2, inflate_ref
from lidar_reference import scan_ref
from mapping_reference import mark_ref, occupancy_ref
from robot_mpcs_amd.global_planner import FREE, OCC

INF = math.inf
MAX_ROBOTS, MAX_TARGETS = 4096, 1024


# ---- targets ---------------------------------------------------------------------------------------------------------
def test_a_tile_with_one_source_and_tiles_without():
    seed = one_seed((7, 5), [2 * 5 + 4])                 # (2, 4): tile (0, 1) of the 3 x 2 tiles of 3 x 3 cells
    targets, tseeds = targets_ref(seed, 3)
    assert targets.tolist() == [-1, 9 + 5, -1, -1, -1, -1]
    assert tseeds.shape == (6, 7, 5) and tseeds[1, 2, 4] == 0.0 and np.isinf(tseeds).sum() == 6 * 35 - 1


def test_centroid_tie_falls_to_the_lower_cell():
    # two sources: both equally far from their centroid; the lower cell index wins
    targets, _ = targets_ref(one_seed((4, 4), [1, 2 * 4 + 3]), 4)
    assert targets.tolist() == [1]
    # a plus: the centre is the centroid itself; a ring of four without the centre: a four-way tie
    plus = [1 * 5 + 2, 2 * 5 + 1, 2 * 5 + 2, 2 * 5 + 3, 3 * 5 + 2]
    assert targets_ref(one_seed((5, 5), plus), 5)[0].tolist() == [2 * 5 + 2]
    assert targets_ref(one_seed((5, 5), [c for c in plus if c != 12]), 5)[0].tolist() == [1 * 5 + 2]
    # an L of three: centroid (1/3, 1/3) from (0, 0), (0, 1), (1, 0): the corner is nearest, n r - Sr exact in integers
    assert targets_ref(one_seed((2, 2), [0, 1, 2]), 2)[0].tolist() == [0]
    # the start potential of a source plays no part: any finite seed is a source
    assert targets_ref(one_seed((4, 4), [1, 11], [7.5, 0.0]), 4)[0].tolist() == [1]


def test_ragged_edge_tiles_one_tile_and_no_source():
    seed = np.full((41, 41), INF)
    seed[40, :] = 0.0                                     # the last row: tiles one cell high
    seed[0, 40] = 0.0                                     # the last column's first tile: one cell wide
    targets, tseeds = targets_ref(seed, 8)
    assert len(targets) == 36 == tiles_of(41, 41, 8)
    assert targets[5] == 40                               # tile (0, 5) = column 40 only
    # tiles (5, j): row 40, columns 8 j .. 8 j + 7: centroid 8 j + 3.5, the lower of the two middle cells
    assert targets[30:35].tolist() == [40 * 41 + 8 * j + 3 for j in range(5)] and targets[35] == 40 * 41 + 40
    assert (targets >= 0).sum() == 7 and all(tseeds[t].ravel()[targets[t]] == 0.0 for t in (5, 30, 35))
    one, ts = targets_ref(seed, 64)
    assert one.shape == (1,) and ts.shape == (1, 41, 41) and np.isfinite(ts).sum() == 1
    assert targets_ref(seed, 41)[0].tolist() == one.tolist()
    none, ts = targets_ref(np.full((41, 41), INF), 8)
    assert none.tolist() == [-1] * 36 and np.all(np.isinf(ts))


# ---- route costs -----------------------------------------------------------------------------------------------------
def test_route_costs_free_occupied_and_outside_starts():
    H0, W0 = 4, 6
    data = np.zeros((H0, W0))
    data[:, 2] = 1.0                                      # a wall: columns 0, 1 | 3 .. 5
    data[0, 5] = 0.5                                      # a graded free cell
    fields = [field_seeded_ref(data, one_seed(data.shape, [0]))[0],
              field_seeded_ref(data, one_seed(data.shape, [0 * W0 + 4]))[0],
              np.full((H0, W0), INF)]                     # the field of a tile without a target
    starts = [3 * W0 + 1, 1 * W0 + 2, -1, H0 * W0, 0 * W0 + 5]
    cost = route_costs_ref(data, fields, starts)
    assert cost.shape == (5, 3) and np.all(np.isinf(cost[:, 2]))
    assert cost[0, 0] == 2.0 + S2 and np.isinf(cost[0, 1])             # a free start: the field's value
    # (1, 2) stands in the wall: field 0 through (1, 1) at 1 + sqrt 2 (or (0, 1) at sqrt 2 + 1), field 1 through (0, 3) or
    # (1, 3) at D = 1: sqrt 2 + 1 against 1 + sqrt 2 -- the same double
    assert np.isinf(fields[0][1, 2]) and cost[1, 0] == 1.0 + S2 and cost[1, 1] == 1.0 + S2
    assert np.all(np.isinf(cost[2])) and np.all(np.isinf(cost[3]))     # outside the map
    # from (0, 5), free: the field's own value, which holds the price 3 * 0 of entering (0, 4), not that of (0, 5)
    assert cost[4, 1] == 1.0 and np.isinf(cost[4, 0])
    # an occupied start prices the neighbour it steps on: walled-in (3, 5) with the graded (2, 5) as its only way out
    data2 = np.zeros((H0, W0))
    data2[3, 5] = data2[3, 4] = data2[2, 4] = 1.0
    data2[2, 5] = 0.5
    D = field_seeded_ref(data2, one_seed(data2.shape, [0 * W0 + 5]))[0]
    assert D[2, 5] == 1.0 + 1.0 and route_costs_ref(data2, [D], [3 * W0 + 5])[0, 0] == 1.0 + (3.0 * 0.5 + 2.0)
    data2[2, 5] = 1.0
    assert np.isinf(route_costs_ref(data2, [field_seeded_ref(data2, one_seed(data2.shape, [5]))[0]], [3 * W0 + 5])[0, 0])


# ---- the assignment --------------------------------------------------------------------------------------------------
def test_greedy_hand_cases():
    # plain greedy matching, not the optimum: (0, 0) at 1 goes first and leaves robot 1 the 10
    a, p = greedy_ref([[1.0, 2.0], [1.5, 10.0]])
    assert a.tolist() == [0, 1] and p.tolist() == [0, 0]
    # ties go by (b, t)
    a, p = greedy_ref(np.zeros((2, 3)))
    assert a.tolist() == [0, 1] and p.tolist() == [0, 0]
    # B > T: the targets are shared out round by round
    cost = np.array([[1.0, 5.0], [2.0, 6.0], [3.0, 0.5], [4.0, 7.0], [9.0, 8.0]])
    a, p = greedy_ref(cost)
    assert a.tolist() == [0, 0, 1, 1, 1] and p.tolist() == [0, 1, 0, 1, 2]
    # a row of +inf stays -1; a column of +inf is never taken; three robots on two usable targets: a second pass
    cost = np.array([[INF, INF, INF], [1.0, INF, 2.0], [3.0, INF, 1.0], [0.5, INF, 4.0]])
    a, p = greedy_ref(cost)
    assert a.tolist() == [-1, 0, 2, 0] and p.tolist() == [-1, 1, 0, 0]
    # NaN and negative entries are never taken; -0.0 is 0
    cost = np.array([[math.nan, -1.0, 3.0], [-INF, -0.0, math.nan], [math.nan, -1e-300, -5.0]])
    a, p = greedy_ref(cost)
    assert a.tolist() == [2, 1, -1] and p.tolist() == [0, 0, -1]
    # nothing takeable: one pass that takes nothing
    a, p = greedy_ref(np.full((3, 2), INF))
    assert a.tolist() == [-1] * 3 and p.tolist() == [-1] * 3
    for cost in ([[1.0, 2.0], [1.5, 10.0]], np.zeros((2, 3)), [[INF] * 3, [1.0, INF, 2.0], [3.0, INF, 1.0], [0.5, INF, 4.0]]):
        for x, y in zip(greedy_ref(cost), greedy_sorted_ref(cost)):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("B,T", [(1, 1), (8, 3), (3, 8), (17, 5), (40, 40), (64, 36), (70, 65), (200, 7)])
@pytest.mark.parametrize("ties", [False, True])
def test_both_restatements_agree(B, T, ties):
    rng = np.random.default_rng(1000 * B + T + ties)
    for _ in range(3):
        cost = random_costs(rng, B, T, ties)
        a, p = greedy_ref(cost)
        a2, p2 = greedy_sorted_ref(cost)
        assert np.array_equal(a, a2) and np.array_equal(p, p2)
        ok = takeable_of(cost)
        assert np.all(ok[np.arange(B)[a >= 0], a[a >= 0]]) and np.all((a >= 0) == (p >= 0))
        for q in range(p.max() + 1):                       # a target at most once per pass
            t = a[p == q]
            assert len(set(t.tolist())) == len(t)
        if B > T >= 2 and not ties:
            assert p.max() >= 1


# ---- kinematic exploration with one target per tile ------------------------------------------------------------------
def explore_coordinated(seed, B, tile=8, max_steps=1500, replan_every=5, rays=64, max_range=10.0):
    """explore_kinematic of tests/exploration_cases.py -- the same store, starts, order of the control step and
    re-plan period -- with the coordinated re-plan: one target per tile of the frontier, a field per target, the route
    costs, the greedy assignment and each robot's descent of the field of its target.  A robot without a target, or with
    a route of length <= 0, keeps the route it has.  Returns what explore_kinematic returns, and the most targets at one
    re-plan and the robot-re-plans that ended without a target."""
    from robot_mpcs_amd.global_planner import png_values
    from robot_mpcs_amd.store import STORE, store_map
    from robot_mpcs_amd.utils.exploration import corner_starts
    from robot_mpcs_amd.utils.lidar import boxes_from_grid
    H, W, cell, x0 = STORE.H, STORE.W, STORE.cell, STORE.x0
    raw = store_map(seed)
    boxes = boxes_from_grid(raw, x0, x0, cell)
    truly_enlarged = inflate_ref(png_values(raw), cell, STORE.size_robot, 0.29)[0] > 0.5
    cells = corner_starts(raw, B).astype(np.int64)
    hits, misses = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    routes, idx = [[int(c)] for c in cells], [0] * B
    ended, on_enlarged, most_targets, unassigned = None, 0, 0, 0
    no_field = np.full((H, W), INF)
    for step in range(max_steps):
        for b in range(B):
            if idx[b] < len(routes[b]) - 1:
                idx[b] += 1
        pose = np.stack([x0 + (cells % W) * cell, x0 + (cells // W) * cell, np.zeros(B)], 1)
        pts, t, _ = scan_ref(pose, rays, -math.pi, math.pi, max_range, (0.0, 0.0), 0.02, boxes)
        org = np.concatenate([pose[:, :2], np.full((B, 1), 0.02)], 1)
        _, _, skipped = mark_ref(org, pts, t, H, W, x0, x0, cell, max_range, 1e-6, hits, misses)
        assert skipped == 0
        if step % replan_every == 0:
            grid, _, _ = occupancy_ref(hits, misses, 3, 1, 0, FREE, OCC, FREE)
            enlarged, _ = inflate_ref(grid, cell, STORE.size_robot, 0.29)
            plan, seeds, count = frontier_ref(hits, misses, enlarged)
            if count == 0:
                ended = step
                break
            targets, tseeds = targets_ref(seeds, tile)
            fields = []
            for g in range(len(targets)):
                D, status = field_seeded_ref(plan, tseeds[g]) if targets[g] >= 0 else (no_field, OK)
                assert status == OK
                fields.append(D)
            assign, _ = greedy_ref(route_costs_ref(plan, fields, cells))
            most_targets = max(most_targets, int((targets >= 0).sum()))
            unassigned += int((assign < 0).sum())
            for b in range(B):
                if assign[b] >= 0:
                    path, n = descend_seeded_ref(plan, fields[assign[b]], tseeds[assign[b]], int(cells[b]),
                                                 max_len=4 * (H + W))
                    if n > 0:
                        routes[b], idx[b] = path, 0
        for b in range(B):
            cells[b] = routes[b][idx[b]]
        on_enlarged += int(truly_enlarged.ravel()[cells].sum())
    free = raw < 0.5
    unseen = free & (hits + misses == 0)
    return dict(ended=ended, free=int(free.sum()), unseen=int(unseen.sum()), on_enlarged=on_enlarged,
                most_targets=most_targets, unassigned=unassigned)


@functools.lru_cache(maxsize=None)
def coordinated(seed, B, tile=8):
    r = explore_coordinated(seed, B, tile)
    print(dict(seed=seed, B=B, tile=tile, **r))
    return r


@pytest.mark.parametrize("seed,B,free", KINEMATIC)
def test_coordinated_kinematic_exploration(seed, B, free):
    """With tile = 8 the run ends, sees every free cell and keeps every robot off the truly enlarged map, as the
    nearest-frontier run of tests/test_exploration_cpu.py does, and it ends no later than that run.  Eight robots must
    end within 0.6 of the nearest-frontier run's steps: steps come in multiples of the re-plan period 5, and the
    restatement gave 45 against 100 (seed 0) and 50 against 125 (seed 3), which leaves two re-plans of slack."""
    base = kinematic(seed, B)
    r = coordinated(seed, B)
    assert r["ended"] is not None and r["ended"] < 1500, r
    assert r["free"] == free and r["unseen"] == 0, r
    assert r["on_enlarged"] == 0, r
    assert r["ended"] <= base["ended"], (r, base)
    if B == 8:
        assert r["ended"] <= 0.6 * base["ended"], (r, base)


# ---- the entries: exported, and their refusals before any HIP call --------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return _lib


def test_new_entries_and_limits_are_exported(lib):
    names = {"rmpc_grid_targets_device", "rmpc_grid_route_costs_device", "rmpc_assign_greedy_device"}
    assert names <= set(lib.EXPORTED_SYMBOLS)
    L = C.CDLL(lib.LIB_PATH)
    assert all(hasattr(L, n) for n in names)
    assert (lib.ASSIGN_MAX_ROBOTS, lib.ASSIGN_MAX_TARGETS) == (MAX_ROBOTS, MAX_TARGETS)
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rmpc.h")).read()
    assert "#define RMPC_ASSIGN_MAX_ROBOTS 4096" in hdr and "#define RMPC_ASSIGN_MAX_TARGETS 1024" in hdr
    assert lib.load_library().rmpc_version() == 201
    assert lib.grid_tiles(41, 41, 8) == 36 and lib.grid_tiles(7, 5, 3) == 6 and lib.grid_tiles(41, 41, 64) == 1


def test_refusals(lib):
    """Each refusal returns -1 with the entry's own message, never the HIP runtime's: host-side fake pointers are never
    dereferenced, and a call that passed validation would report a HIP error on a machine without a device."""
    L = lib.load_library()
    P = C.c_void_p(0x1000)
    nan, inf = math.nan, math.inf

    def targets(H=41, W=41, seed=P, tile=8, cells=P, tseeds=P):
        rc = L.rmpc_grid_targets_device(H, W, seed, tile, cells, tseeds, None)
        return rc, L.rmpc_last_error().decode()

    cases = [(dict(seed=None), "null argument"), (dict(cells=None), "null argument"), (dict(H=0), "need H, W >= 1"),
             (dict(W=-3), "need H, W >= 1"), (dict(H=129, W=128), "RMPC_GRID_MAX_CELLS"),
             (dict(H=1 << 16, W=1 << 16), "RMPC_GRID_MAX_CELLS"), (dict(tile=0), "tile >= 1"), (dict(tile=-8), "tile >= 1"),
             (dict(tile=1), "RMPC_ASSIGN_MAX_TARGETS"), (dict(H=128, W=128, tile=3), "RMPC_ASSIGN_MAX_TARGETS"),
             (dict(H=33, W=32, tile=1, tseeds=None), "RMPC_ASSIGN_MAX_TARGETS")]
    for kw, want in cases:
        rc, msg = targets(**kw)
        assert rc == -1 and want in msg and "hip" not in msg.lower(), (kw, msg)

    def costs(H=41, W=41, grid=P, T=36, fields=P, B=64, start=P, mv=8, occ=0.8, f=3.0, cost=P):
        rc = L.rmpc_grid_route_costs_device(H, W, grid, T, fields, B, start, mv, occ, f, cost, None)
        return rc, L.rmpc_last_error().decode()

    cases = [(dict(grid=None), "null argument"), (dict(fields=None), "null argument"), (dict(start=None), "null argument"),
             (dict(cost=None), "null argument"), (dict(H=0), "need H, W >= 1"), (dict(W=0), "need H, W >= 1"),
             (dict(mv=5), "movement must be 4 or 8"), (dict(B=0), "RMPC_ASSIGN_MAX_ROBOTS"),
             (dict(B=MAX_ROBOTS + 1), "RMPC_ASSIGN_MAX_ROBOTS"), (dict(T=0), "RMPC_ASSIGN_MAX_TARGETS"),
             (dict(T=MAX_TARGETS + 1), "RMPC_ASSIGN_MAX_TARGETS"), (dict(H=2048, W=2048, T=1024), "INT_MAX"),
             (dict(f=-1.0), "cost_factor"), (dict(f=nan), "cost_factor"), (dict(f=inf), "cost_factor")]
    for kw, want in cases:
        rc, msg = costs(**kw)
        assert rc == -1 and want in msg and "hip" not in msg.lower(), (kw, msg)

    def assign(B=64, T=36, cost=P, out=P, passes=P):
        rc = L.rmpc_assign_greedy_device(B, T, cost, out, passes, None)
        return rc, L.rmpc_last_error().decode()

    cases = [(dict(cost=None), "null argument"), (dict(out=None), "null argument"), (dict(B=0), "RMPC_ASSIGN_MAX_ROBOTS"),
             (dict(B=-1, passes=None), "RMPC_ASSIGN_MAX_ROBOTS"), (dict(B=MAX_ROBOTS + 1), "RMPC_ASSIGN_MAX_ROBOTS"),
             (dict(T=0), "RMPC_ASSIGN_MAX_TARGETS"), (dict(T=MAX_TARGETS + 1), "RMPC_ASSIGN_MAX_TARGETS")]
    for kw, want in cases:
        rc, msg = assign(**kw)
        assert rc == -1 and want in msg and "hip" not in msg.lower(), (kw, msg)


def test_frontier_goals_refuses_a_tile_or_fleet_beyond_the_limits(lib):
    """before any tensor is made: no device is needed"""
    from types import SimpleNamespace
    from robot_mpcs_amd.utils.exploration import FrontierGoals
    fmap = SimpleNamespace(H=41, W=41, B=8, device="cpu")
    with pytest.raises(ValueError, match="RMPC_ASSIGN_MAX_TARGETS"):
        FrontierGoals(fmap, 0.45, tile=1)
    with pytest.raises(ValueError, match="tile must be >= 0"):
        FrontierGoals(fmap, 0.45, tile=-1)
    fmap.B = MAX_ROBOTS + 1
    with pytest.raises(ValueError, match="RMPC_ASSIGN_MAX_ROBOTS"):
        FrontierGoals(fmap, 0.45, tile=8)
