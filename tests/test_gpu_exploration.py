"""Frontier exploration on the device (rmpc_grid_frontier_device, rmpc_grid_fields_seeded_device,
rmpc_grid_descend_device, FrontierGoals) against the numpy restatements of tests/exploration_reference.py; the seeded
field against rmpc_grid_fields_device, bit for bit; stream ordering; the closed loop of
examples/fleet_store_frontier.py."""
import math

import numpy as np
import pytest

from example_loader import load_example
from exploration_cases import evidence, grid_of, one_seed
from exploration_reference import (BAD_MAP, BAD_SEED, OK, OUTSIDE, TOO_LONG, descend_seeded_ref, field_seeded_ref,
                                   frontier_ref)
from global_planner_reference import inflate_ref
from gpu_support import DEV, _t
from mapping_reference import occupancy_ref
from robot_mpcs_amd.global_planner import FREE, OCC

pytestmark = pytest.mark.gpu

INF = math.inf


@pytest.fixture(scope="module")
def rt():
    import torch
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return dict(torch=torch, lib=_lib)


# ---- the frontier ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (3, 3), (37, 53), (41, 41), (128, 128)])
@pytest.mark.parametrize("kind", ["sparse", "unknown", "known"])
def test_frontier_matches_restatement(rt, H, W, kind):
    torch, lib = rt["torch"], rt["lib"]
    rng = np.random.default_rng(H * 1000 + W)
    hits, misses, enlarged = evidence(H, W, kind, rng)
    th, tm, te = _t(torch, hits, torch.int32), _t(torch, misses, torch.int32), _t(torch, enlarged)
    total = 0
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    for nmoves, unknown_value in ((4, 1.0), (8, 0.9)):
        plan = torch.full((H, W), float("nan"), dtype=torch.float64, device=DEV)
        seed = torch.full((H, W), float("nan"), dtype=torch.float64, device=DEV)
        lib.grid_frontier_device(th, tm, te, plan, seed, count, 0.8, nmoves, unknown_value)
        rp, rs, rc = frontier_ref(hits, misses, enlarged, 0.8, nmoves, unknown_value)
        total += rc                                      # the second call adds to a count that was not zeroed
        assert np.array_equal(plan.cpu().numpy(), rp) and np.array_equal(seed.cpu().numpy(), rs)
        assert int(count.item()) == total
        if kind != "sparse":
            assert rc == 0
    if kind == "sparse" and H * W > 9:
        assert total > 0
    assert torch.equal(th, _t(torch, hits, torch.int32)) and torch.equal(tm, _t(torch, misses, torch.int32))


# ---- the seeded field --------------------------------------------------------------------------------------------------
def seeds_of(data, G, seed):
    """G seed grids: 1 .. 12 sources each on free cells, a third of them with a start potential in [0, 6), two seeds on
    occupied cells"""
    rng = np.random.default_rng(seed)
    free, occ = np.flatnonzero(data.ravel() < 0.8), np.flatnonzero(data.ravel() >= 0.8)
    out = np.full((G,) + data.shape, INF)
    for g in range(G):
        cells = rng.choice(free, min(len(free), int(rng.integers(1, 13))), replace=False)
        out[g].ravel()[cells] = np.where(rng.uniform(size=len(cells)) < 0.33, rng.uniform(0.0, 6.0, len(cells)), 0.0)
        if len(occ):
            out[g].ravel()[rng.choice(occ, min(len(occ), 2), replace=False)] = [0.0, -1.0][:min(len(occ), 2)]
    return out


def run_seeded(rt, data, seeds, movement=8):
    torch, lib = rt["torch"], rt["lib"]
    G = seeds.shape[0]
    fields = torch.full(seeds.shape, float("nan"), dtype=torch.float64, device=DEV)
    status = torch.full((G,), 99, dtype=torch.int32, device=DEV)
    sweeps = torch.full((G,), -1, dtype=torch.int32, device=DEV)
    lib.grid_fields_seeded_device(_t(torch, data), _t(torch, seeds), fields, status, movement, 0.8, 3.0, sweeps=sweeps)
    return fields.cpu().numpy(), status.cpu().numpy(), sweeps.cpu().numpy()


def run_goal_fields(rt, data, goals, movement=8):
    torch, lib = rt["torch"], rt["lib"]
    G = len(goals)
    fields = torch.full((G,) + data.shape, float("nan"), dtype=torch.float64, device=DEV)
    status = torch.full((G,), 99, dtype=torch.int32, device=DEV)
    lib.grid_fields_device(_t(torch, data), _t(torch, goals, torch.int32), fields, status, movement, 0.8, 3.0)
    assert bool((status == 0).all())
    return fields.cpu().numpy()


def same_field(got, ref, exact):
    """bitwise, or the existing bar on graded maps: the same cells finite, 1e-12 relative on them"""
    if exact:
        return np.array_equal(got, ref)
    fin = np.isfinite(ref)
    return np.array_equal(np.isfinite(got), fin) and np.all(np.abs(got[fin] - ref[fin]) <= 1e-12 * np.abs(ref[fin]))


# shapes: one cell; one row; fewer cells than threads; 1961 cells (runs of 3 cells, the last threads idle); 16384 cells
# (runs of 17, every thread busy).  G = 64 only where the heap restatement takes milliseconds.
@pytest.mark.parametrize("H,W,kind,G,movement", [
    (1, 1, "binary", 1, 8), (1, 7, "graded", 3, 8), (3, 3, "binary", 3, 4), (37, 53, "binary", 64, 8),
    (37, 53, "graded", 64, 8), (41, 41, "store", 3, 8), (41, 41, "graded", 3, 4), (128, 128, "store", 3, 8),
    (128, 128, "graded", 1, 8)])
def test_seeded_fields_match_the_heap_restatement(rt, H, W, kind, G, movement):
    data = grid_of(H, W, kind, 7 * H + W)
    if H * W == 1:
        data[:] = 0.0
    seeds = seeds_of(data, G, H + W + G)
    got, status, sweeps = run_seeded(rt, data, seeds, movement)
    for g in range(G):
        ref, st = field_seeded_ref(data, seeds[g], movement)
        assert st == OK == status[g] and 1 <= sweeps[g] <= H * W + 1
        assert same_field(got[g], ref, kind != "graded"), (g, np.nanmax(np.abs(got[g] - ref)))
        assert np.all(np.isinf(got[g][data >= 0.8]))


@pytest.mark.parametrize("H,W,kind", [(41, 41, "store"), (37, 53, "graded"), (128, 128, "store"), (128, 128, "graded")])
def test_seeded_field_equals_the_goal_fields_bit_for_bit(rt, H, W, kind):
    """seed 0 at one cell: the existing entry's field of that goal; seed 0 at five cells: the element-wise minimum of
    its five fields.  Both are the minimum over the same path values, each the same nested expression."""
    data = grid_of(H, W, kind, 11 * H + W)
    rng = np.random.default_rng(H + W)
    goals = rng.choice(np.flatnonzero(data.ravel() < 0.8), 5, replace=False).astype(np.int32)
    goal_fields = run_goal_fields(rt, data, goals)
    seeds = np.stack([one_seed(data.shape, [goals[0]]), one_seed(data.shape, goals)])
    got, status, _ = run_seeded(rt, data, seeds)
    assert status.tolist() == [OK, OK]
    assert np.array_equal(got[0], goal_fields[0])
    assert np.array_equal(got[1], goal_fields.min(axis=0))
    assert np.isfinite(got[1]).sum() > 0.5 * (data < 0.8).sum()


def test_seed_rules_on_the_device(rt):
    """one launch of six fields: no finite seed; seeds on occupied cells only; a potential that a neighbour undercuts and
    one that stays a source; a negative seed; a NaN seed; an ordinary field.  The bad fields end with RMPC_GRID_BAD_SEED,
    all +inf and 0 sweeps, and leave the others as they are."""
    data = grid_of(41, 41, "store", 0)
    free, occ = np.flatnonzero(data.ravel() < 0.8), np.flatnonzero(data.ravel() >= 0.8)
    a = int(free[len(free) // 2])
    assert data.ravel()[a + 1] < 0.8
    seeds = np.full((6, 41, 41), INF)
    seeds[1].ravel()[occ[:5]] = [0.0, 1.0, -1.0, math.nan, -INF]
    seeds[2].ravel()[[a, a + 1, int(free[3])]] = [0.0, 5.0, 0.25]
    seeds[3].ravel()[[a, int(free[7])]] = [0.0, -1e-300]
    seeds[4].ravel()[[a, int(free[9])]] = [0.0, math.nan]
    seeds[5].ravel()[a] = 0.0
    got, status, sweeps = run_seeded(rt, data, seeds)
    assert status.tolist() == [OK, OK, OK, BAD_SEED, BAD_SEED, OK]
    assert np.all(np.isinf(got[[0, 1, 3, 4]])) and sweeps[[0, 1]].tolist() == [1, 1] and sweeps[[3, 4]].tolist() == [0, 0]
    assert got[2].ravel()[a] == 0.0 and got[2].ravel()[a + 1] == 1.0 and got[2].ravel()[int(free[3])] == 0.25
    for g in (2, 5):
        ref, st = field_seeded_ref(data, seeds[g])
        assert st == OK and np.array_equal(got[g], ref)
    # a negative free cell of the map comes first, as in rmpc_grid_fields_device
    data.ravel()[int(free[0])] = -0.5
    got, status, sweeps = run_seeded(rt, data, seeds[3:])
    assert status.tolist() == [BAD_MAP] * 3 and np.all(np.isinf(got)) and sweeps.tolist() == [0, 0, 0]


# ---- the descent -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def descent_case(rt):
    """the 128 x 128 store, two seeded fields (60 sources with potentials; 3 sources), 4099 robots: most on random cells,
    occupied ones included, the first ones on sources, some outside the map or with a field index outside [0, G)"""
    data = grid_of(128, 128, "store", 0)
    rng = np.random.default_rng(21)
    free = np.flatnonzero(data.ravel() < 0.8)
    seeds = np.full((2, 128, 128), INF)
    src = rng.choice(free, 60, replace=False)
    seeds[0].ravel()[src] = np.where(rng.uniform(size=60) < 0.3, rng.uniform(0.0, 8.0, 60), 0.0)
    seeds[1].ravel()[rng.choice(free, 3, replace=False)] = 0.0
    # a pocket no source reaches: a free cell walled in (an unreachable start), beside it a wall cell whose only free
    # neighbour is that cell (an occupied start without a finite neighbour)
    r, c = np.argwhere(data[2:-2, 2:-2] < 0.8)[0] + 2
    data[r - 1:r + 2, c - 1:c + 2] = 1.0
    data[r, c] = 0.0
    seeds[:, r - 1:r + 2, c - 1:c + 2] = INF
    B = 4099
    start = rng.integers(0, 128 * 128, B).astype(np.int32)
    fi = (rng.uniform(size=B) < 0.03).astype(np.int32)
    start[:60], fi[:60] = src, 0
    start[60:64] = [-1, 128 * 128, -7, 1 << 30]
    fi[64:68] = [-1, 2, 99, -5]
    start[68], start[69] = r * 128 + c, (r - 1) * 128 + c
    fields, status, _ = run_seeded(rt, data, seeds)
    assert status.tolist() == [OK, OK]
    for g in range(2):
        assert np.array_equal(fields[g], field_seeded_ref(data, seeds[g])[0])
    return dict(data=data, seeds=seeds, fields=fields, start=start, fi=fi)


def run_descend(rt, case, max_len):
    torch, lib = rt["torch"], rt["lib"]
    B = len(case["start"])
    path = torch.full((B, max_len), -9, dtype=torch.int32, device=DEV)
    length = torch.full((B,), 99, dtype=torch.int32, device=DEV)
    lib.grid_descend_device(_t(torch, case["data"]), _t(torch, case["fields"]), _t(torch, case["seeds"]),
                            _t(torch, case["start"], torch.int32), _t(torch, case["fi"], torch.int32), path, length, 8,
                            0.8, 3.0)
    return path.cpu().numpy(), length.cpu().numpy()


@pytest.mark.parametrize("max_len", [512, 6])
def test_descent_matches_restatement(rt, descent_case, max_len):
    """paths and lengths exactly those of the restatement; cells past the length (or, for a length <= 0 other than
    RMPC_GRID_TOO_LONG, any cell) are not written"""
    case = descent_case
    path, length = run_descend(rt, case, max_len)
    data, start, fi = case["data"], case["start"], case["fi"]
    kinds = dict(source=0, occupied_start=0, too_long=0, unreachable=0, outside=0, passed_through=0)
    for b in range(len(start)):
        if not 0 <= fi[b] < 2:
            cells, n = [], OUTSIDE
        else:
            cells, n = descend_seeded_ref(data, case["fields"][fi[b]], case["seeds"][fi[b]], int(start[b]), max_len=max_len)
        assert length[b] == n, (b, length[b], n)
        assert path[b, :len(cells)].tolist() == cells and np.all(path[b, len(cells):] == -9), b
        kinds["source"] += n == 1
        kinds["too_long"] += n == TOO_LONG
        kinds["unreachable"] += n == 0
        kinds["outside"] += n == OUTSIDE
        if n > 1:
            kinds["occupied_start"] += data.ravel()[start[b]] >= 0.8
            kinds["passed_through"] += bool(np.isfinite(case["seeds"][fi[b]].ravel()[cells[:-1]]).any())
    print(kinds)
    assert length[68] == 0 and length[69] == 0 and kinds["outside"] >= 8 and kinds["source"] >= 40
    assert kinds["occupied_start"] > 100 and kinds["unreachable"] >= 2 and kinds["passed_through"] >= 1
    assert (kinds["too_long"] > 100) == (max_len == 6) and (kinds["too_long"] == 0) == (max_len == 512)


# ---- FrontierGoals: the chain, and its order on a stream ---------------------------------------------------------------
def test_frontier_goals_chain_and_stream_ordering(rt):
    """FrontierGoals.replan after one marked scan of 64 robots in the 41 x 41 store against the chain of restatements,
    then on a side stream: its launches and tensor operations are ordered on the stream it is given"""
    from robot_mpcs_amd.global_planner import RouteFollower, shelf_map
    from robot_mpcs_amd.utils.exploration import FrontierGoals, corner_starts
    from robot_mpcs_amd.utils.lidar import LidarPlanes, boxes_from_grid
    from robot_mpcs_amd.utils.mapping import FleetMap
    torch = rt["torch"]
    H = W = 41
    cell, x0, B = 0.45, -9.0, 64
    raw = shelf_map(H, W, seed=0, aisle=6, shelf=2, gap=5)
    starts = corner_starts(raw, B)
    rng = np.random.default_rng(2)
    pose = np.zeros((B, 8))
    pose[:, 0], pose[:, 1] = x0 + (starts % W) * cell, x0 + (starts // W) * cell
    pose[:, 2] = rng.uniform(-math.pi, math.pi, B)
    pose[5, :2] = 100.0                                    # a robot outside the map keeps its route
    tx = _t(torch, pose)
    lp = LidarPlanes(B, 3, 2, boxes=boxes_from_grid(raw, x0, x0, cell), device=DEV)
    fmap = FleetMap(B, H, W, x0, x0, cell, 64, lp.max_range, lp.offset, lp.height, device=DEV)
    fg = FrontierGoals(fmap, 0.45, 0.29)
    old = torch.arange(B * fg.max_len, dtype=torch.int32, device=DEV).reshape(B, fg.max_len) % (H * W)

    def chain(stream):
        with torch.cuda.stream(stream):
            fmap.reset()
            for t in (fg.enlarged, fg.plan, fg.seed, fg.field):
                t.fill_(float("nan"))
            fg.lens.fill_(77)
            fg.paths.fill_(-1)
            fg.count.fill_(123)
            fol = RouteFollower(old.clone(), torch.full((B,), 3, dtype=torch.int32, device=DEV), W, x0, x0, cell)
            fol.idx.fill_(2)
            lp.step(tx)
            fmap.mark(tx, lp.points, lp.ranges)
            fg.replan(fol, tx, stream=stream)
        n = fg.frontier_cells()
        return [n] + [t.cpu().numpy().copy() for t in (fmap.hits, fmap.misses, fg.enlarged, fg.plan, fg.seed, fg.field,
                                                        fg.status, fg.cells, fg.lens, fol.paths, fol.lens, fol.idx)]

    ref = chain(torch.cuda.default_stream(0))
    n, hits, misses, enlarged, plan, seed, field, status, cells, lens, fpaths, flens, fidx = ref
    grid, _, _ = occupancy_ref(hits, misses, 3, 1, 0, FREE, OCC, FREE)
    r_enl, _ = inflate_ref(grid, cell, 0.45, 0.29)
    r_plan, r_seed, r_n = frontier_ref(hits, misses, r_enl)
    r_field, r_st = field_seeded_ref(r_plan, r_seed)
    assert np.array_equal(enlarged, r_enl) and np.array_equal(plan, r_plan) and np.array_equal(seed, r_seed)
    assert n == r_n > 0 and status[0] == r_st == OK and np.array_equal(field[0], r_field)
    assert cells[5] == -1 and np.array_equal(np.delete(cells, 5), np.delete(starts, 5))
    for b in range(B):
        want, m = descend_seeded_ref(r_plan, r_field, r_seed, int(cells[b]), max_len=fg.max_len)
        assert lens[b] == m, (b, lens[b], m)
        if m > 0:
            assert flens[b] == m and fidx[b] == 0 and fpaths[b, :m].tolist() == want
        else:
            assert flens[b] == 3 and fidx[b] == 2 and np.array_equal(fpaths[b], old[b].cpu().numpy())
    assert lens[5] == OUTSIDE and (lens > 1).sum() > B // 2
    side = torch.cuda.Stream(device=0)
    for _ in range(3):
        got = chain(side)
        assert got[0] == ref[0] and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ref[1:], got[1:]))


# ---- the closed loop ---------------------------------------------------------------------------------------------------
MEASURED_END_STEP = 80   # MI355X, seed 0, B = 64: the first re-plan without a frontier


def test_closed_loop_fleet_explores_the_store(rt):
    """64 boxers without a map or goals explore the store of examples/fleet_store_lidar.py from one corner
    (examples/fleet_store_frontier.py, seed 0, at most 3000 control steps, a re-plan every 10).  Gates: exploration ends
    (a re-plan finds no frontier); at most 0.5 % of the store's free cells are unseen then (a condition; the kinematic
    restatement leaves none); the lidar loop's safety gates (at most 1 % failed robot-steps, no base centre inside a
    shelf, the end link at least 0.5 r_body from every shelf); and the ending step by 1.35 x the one measured on the
    MI355X, the margin the other loops use for run-to-run changes of the solver's constants.  Measured there: the run
    ends at step 80 (the ninth re-plan) with 1371 of 1371 free cells seen, none of the 1677 seen cells classified
    against the truth, no failed solve, the end link 0.590 m and the base 0.203 m from the nearest shelf."""
    ex = load_example("fleet_store_frontier")
    r = ex.run(B=64, seed=0, steps=3000)
    print(r)
    assert r["fused"]
    assert r["ended_step"] is not None and r["frontier_cells"] == 0, r
    assert r["free_cells"] - r["free_cells_seen"] <= 0.005 * r["free_cells"], r
    assert r["failed_share"] <= 0.01, r
    assert r["base_inside"] == 0 and r["min_base_clearance_m"] > 0.0, r
    assert r["min_ee_clearance_m"] >= 0.5 * r["r_body"], r
    assert r["ended_step"] <= 1.35 * MEASURED_END_STEP, r
