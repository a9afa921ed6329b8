"""Coordinated exploration on the device (rmpc_grid_targets_device, rmpc_grid_route_costs_device,
rmpc_assign_greedy_device, FrontierGoals(tile=...)) against the numpy restatements of tests/assignment_reference.py, bit
for bit; stream ordering; the closed loop of examples/fleet_store_frontier.py with and without coordination."""
import math

import numpy as np
import pytest

from assignment_cases import random_costs
from assignment_reference import greedy_ref, greedy_sorted_ref, route_costs_ref, targets_ref, tiles_of
from example_loader import load_example
from exploration_cases import evidence, grid_of
from exploration_reference import OK, OUTSIDE, descend_seeded_ref, field_seeded_ref, frontier_ref
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


# ---- targets ---------------------------------------------------------------------------------------------------------
def seed_grid(H, W, kind, rng):
    """"binary": a fifth of the cells are sources, some with a start potential; "frontier": the frontier of sparse random
    evidence (tests/exploration_cases.py); "none": no source"""
    if kind == "none":
        return np.full((H, W), INF)
    if kind == "frontier":
        hits, misses, enlarged = evidence(H, W, "sparse", rng)
        seed = frontier_ref(hits, misses, enlarged)[1]
        assert np.isfinite(seed).sum() > 0
        return seed
    return np.where(rng.uniform(size=(H, W)) < 0.2, np.where(rng.uniform(size=(H, W)) < 0.5, 0.0, 2.5), INF)


@pytest.mark.parametrize("H,W,tile,kind", [
    (7, 5, 3, "binary"), (41, 41, 8, "frontier"), (41, 41, 8, "binary"), (41, 41, 5, "frontier"), (32, 32, 1, "binary"),
    (128, 128, 8, "frontier"), (128, 128, 8, "binary"), (41, 41, 8, "none"), (37, 53, 64, "binary")])
def test_targets_match_restatement(rt, H, W, tile, kind):
    """every tile's target and the whole of tseeds, written into poisoned buffers; tseeds NULL changes nothing else"""
    torch, lib = rt["torch"], rt["lib"]
    seed = seed_grid(H, W, kind, np.random.default_rng(H * 1000 + W + tile))
    T = tiles_of(H, W, tile)
    assert T == lib.grid_tiles(H, W, tile)
    want, want_seeds = targets_ref(seed, tile)
    ts = _t(torch, seed)
    cells = torch.full((T,), -7, dtype=torch.int32, device=DEV)
    lib.grid_targets_device(ts, tile, cells)
    assert np.array_equal(cells.cpu().numpy(), want)
    cells.fill_(-9)
    tseeds = torch.full((T, H, W), float("nan"), dtype=torch.float64, device=DEV)
    lib.grid_targets_device(ts, tile, cells, tseeds)
    assert np.array_equal(cells.cpu().numpy(), want) and np.array_equal(tseeds.cpu().numpy(), want_seeds)
    assert ((want >= 0).sum() == 0) == (kind == "none") and torch.equal(ts, _t(torch, seed))
    if (H, W, tile) == (32, 32, 1):
        assert T == 1024 and np.array_equal(want >= 0, np.isfinite(seed).ravel())
    with pytest.raises(ValueError):
        lib.grid_targets_device(ts, tile, torch.zeros(T + 1, dtype=torch.int32, device=DEV))


# ---- route costs -----------------------------------------------------------------------------------------------------
def test_route_costs_match_restatement(rt):
    """41 x 41 store, T = 36 with the tiles of the upper rows empty (their fields are all +inf), B = 64 robots on free
    cells, shelf cells, cells with shelf all around, and outside the map"""
    torch, lib = rt["torch"], rt["lib"]
    H = W = 41
    data = grid_of(H, W, "store", 0)
    data[19:24, 19:24] = 1.0                               # a block of shelf: (21, 21) has no free cell around it
    rng = np.random.default_rng(8)
    free, occ = np.flatnonzero(data.ravel() < 0.8), np.flatnonzero(data.ravel() >= 0.8)
    seed = np.full(H * W, INF)
    seed[rng.choice(free[free >= 16 * W], 120, replace=False)] = 0.0
    seed[occ[occ >= 16 * W][::7]] = 0.0                    # sources on shelf cells: a target there has an all +inf field
    targets, tseeds = targets_ref(seed.reshape(H, W), 8)
    T, B = 36, 64
    assert len(targets) == T and (targets[:12] == -1).all() and (targets >= 0).sum() >= 18
    fields = torch.full((T, H, W), float("nan"), dtype=torch.float64, device=DEV)
    status = torch.full((T,), 99, dtype=torch.int32, device=DEV)
    lib.grid_fields_seeded_device(_t(torch, data), _t(torch, tseeds), fields, status)
    F = fields.cpu().numpy()
    assert (status == 0).all() and np.all(np.isinf(F[:12]))
    for t in (12, 20, 35):
        assert np.array_equal(F[t], field_seeded_ref(data, tseeds[t])[0])
    start = rng.choice(free, B).astype(np.int32)
    start[:24] = rng.choice(occ, 24)
    start[24:26] = [21 * W + 21, 22 * W + 21]
    start[26:31] = [-1, H * W, -5, 1 << 30, H * W - 1]
    for movement in (8, 4):
        if movement == 4:
            lib.grid_fields_seeded_device(_t(torch, data), _t(torch, tseeds), fields, status, movement)
            F = fields.cpu().numpy()
        cost = torch.full((B, T), float("nan"), dtype=torch.float64, device=DEV)
        lib.grid_route_costs_device(_t(torch, data), fields, _t(torch, start, torch.int32), cost, movement)
        want = route_costs_ref(data, F, start, movement)
        got = cost.cpu().numpy()
        assert np.array_equal(got, want)
        assert np.all(np.isinf(got[24:30])) and np.all(np.isinf(got[:, :12]))
        stepped_out = np.isfinite(got[:24]).any(axis=1).sum()
        assert stepped_out >= 12 and np.isfinite(got[31:]).sum() > 100, stepped_out


# ---- the assignment --------------------------------------------------------------------------------------------------
def run_assign(rt, cost, poison, with_pass=True):
    torch, lib = rt["torch"], rt["lib"]
    B = cost.shape[0]
    assign = torch.full((B,), poison, dtype=torch.int32, device=DEV)
    passes = torch.full((B,), poison + 1, dtype=torch.int32, device=DEV) if with_pass else None
    tc = _t(torch, cost)
    lib.assign_greedy_device(tc, assign, passes)
    assert np.array_equal(tc.cpu().numpy(), cost, equal_nan=True)
    return assign.cpu().numpy(), passes.cpu().numpy() if with_pass else None


# (70, 65): the targets cross a wave; (1025, 5): some threads hold two robots, 200 and more passes; (1024, 256) and
# (4096, 64): several rows per step of the column sweep and many passes
@pytest.mark.parametrize("B,T", [(1, 1), (8, 3), (3, 8), (64, 36), (70, 65), (256, 256), (1025, 5), (1024, 256),
                                 (4096, 64), (5, 1024)])
@pytest.mark.parametrize("ties", [False, True])
def test_assignment_matches_the_sequential_rule(rt, B, T, ties):
    cost = random_costs(np.random.default_rng(77 * B + T + ties), B, T, ties)
    want_a, want_p = greedy_sorted_ref(cost)
    if B * T <= 70 * 65:
        ref_a, ref_p = greedy_ref(cost)
        assert np.array_equal(ref_a, want_a) and np.array_equal(ref_p, want_p)
    a1, p1 = run_assign(rt, cost, -77)
    a2, p2 = run_assign(rt, cost, 123456)
    a3, _ = run_assign(rt, cost, 5, with_pass=False)
    assert np.array_equal(a1, a2) and np.array_equal(p1, p2) and np.array_equal(a1, a3)
    assert np.array_equal(a1, want_a), np.flatnonzero(a1 != want_a)[:8]
    assert np.array_equal(p1, want_p), np.flatnonzero(p1 != want_p)[:8]
    if B > 2 * T and T > 1:
        assert want_p.max() >= 2
    if B * T >= 16:
        assert (want_a == -1).any() and (want_a >= 0).any()         # the rows of +inf; the others


def test_assignment_edge_matrices(rt):
    """nothing takeable; a single column shared out over B passes; all costs equal (one pair per round)"""
    for cost in (np.full((9, 4), INF), np.full((3, 3), math.nan), -np.ones((4, 2)), np.arange(40.0)[::-1].reshape(40, 1),
                 np.zeros((130, 70)), np.zeros((70, 130))):
        want_a, want_p = greedy_ref(cost)
        a, p = run_assign(rt, cost, -3)
        assert np.array_equal(a, want_a) and np.array_equal(p, want_p)


# ---- FrontierGoals(tile): the chain, and its order on a stream -------------------------------------------------------
def test_coordinated_chain_and_stream_ordering(rt):
    """FrontierGoals(tile=8).replan after one marked scan of 64 robots in a corner of the 41 x 41 store against the
    composed restatements, then on a side stream; FrontierGoals(tile=0) beside it against FrontierGoals()"""
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
    fg = FrontierGoals(fmap, 0.45, 0.29, tile=8)
    T = 36
    assert fg.T == T and fg.targets.shape == (T,) and fg.tseeds.shape == fg.fields.shape == (T, H, W)
    assert fg.status.shape == fg.sweeps.shape == (T,) and fg.cost.shape == (B, T) and fg.assign.shape == fg.passes.shape == (B,)
    old = torch.arange(B * fg.max_len, dtype=torch.int32, device=DEV).reshape(B, fg.max_len) % (H * W)

    def chain(g, stream, names):
        with torch.cuda.stream(stream):
            fmap.reset()
            for name in names:
                t = getattr(g, name)
                t.fill_(float("nan") if t.dtype == torch.float64 else 77)
            fol = RouteFollower(old.clone(), torch.full((B,), 3, dtype=torch.int32, device=DEV), W, x0, x0, cell)
            fol.idx.fill_(2)
            lp.step(tx)
            fmap.mark(tx, lp.points, lp.ranges)
            g.replan(fol, tx, stream=stream)
        n = g.frontier_cells()
        return [n] + [t.cpu().numpy().copy() for t in [fmap.hits, fmap.misses, fol.paths, fol.lens, fol.idx]
                      + [getattr(g, name) for name in names]]

    names = ["enlarged", "plan", "seed", "targets", "tseeds", "fields", "status", "cells", "cost", "assign", "passes",
             "lens", "paths"]
    ref = chain(fg, torch.cuda.default_stream(0), names)
    n, hits, misses, fpaths, flens, fidx = ref[:6]
    got = dict(zip(names, ref[6:]))
    grid, _, _ = occupancy_ref(hits, misses, 3, 1, 0, FREE, OCC, FREE)
    r_enl, _ = inflate_ref(grid, cell, 0.45, 0.29)
    r_plan, r_seed, r_n = frontier_ref(hits, misses, r_enl)
    r_targets, r_tseeds = targets_ref(r_seed, 8)
    assert n == r_n > 0 and np.array_equal(got["plan"], r_plan) and np.array_equal(got["seed"], r_seed)
    assert np.array_equal(got["targets"], r_targets) and np.array_equal(got["tseeds"], r_tseeds)
    assert 2 <= (r_targets >= 0).sum() < T
    r_fields = np.full((T, H, W), INF)
    for t in np.flatnonzero(r_targets >= 0):
        r_fields[t], st = field_seeded_ref(r_plan, r_tseeds[t])
        assert st == OK
    assert (got["status"] == OK).all() and np.array_equal(got["fields"], r_fields)
    cells = got["cells"]
    assert cells[5] == -1 and np.array_equal(np.delete(cells, 5), np.delete(starts, 5))
    r_cost = route_costs_ref(r_plan, r_fields, cells)
    assert np.array_equal(got["cost"], r_cost)
    r_assign, r_passes = greedy_ref(r_cost)
    assert np.array_equal(got["assign"], r_assign) and np.array_equal(got["passes"], r_passes)
    assert r_assign[5] == -1 and (np.delete(r_assign, 5) >= 0).all() and r_passes.max() >= 1
    lens = got["lens"]
    for b in range(B):
        if r_assign[b] < 0:
            want, m = [], OUTSIDE
        else:
            want, m = descend_seeded_ref(r_plan, r_fields[r_assign[b]], r_tseeds[r_assign[b]], int(cells[b]),
                                         max_len=fg.max_len)
        assert lens[b] == m, (b, lens[b], m)
        if m > 0:
            assert flens[b] == m and fidx[b] == 0 and fpaths[b, :m].tolist() == want and want[-1] == r_targets[r_assign[b]]
        else:
            assert flens[b] == 3 and fidx[b] == 2 and np.array_equal(fpaths[b], old[b].cpu().numpy())
    assert lens[5] == OUTSIDE and (lens > 1).sum() > B // 2
    side = torch.cuda.Stream(device=0)
    for _ in range(3):
        again = chain(fg, side, names)
        assert again[0] == ref[0] and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ref[1:], again[1:]))
    # tile = 0 is the object without the argument
    names0 = ["enlarged", "plan", "seed", "field", "status", "sweeps", "cells", "lens", "paths"]
    plain, zero = FrontierGoals(fmap, 0.45, 0.29), FrontierGoals(fmap, 0.45, 0.29, tile=0)
    assert sorted(vars(plain)) == sorted(vars(zero)) and zero.tile == 0 and not hasattr(zero, "targets")
    ra, rb = chain(plain, side, names0), chain(zero, side, names0)
    assert ra[0] == rb[0] == n and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ra[1:], rb[1:]))
    assert np.array_equal(ra[6 + names0.index("seed")], r_seed) and (ra[6 + names0.index("lens")] > 1).sum() > B // 2


# ---- the closed loop -------------------------------------------------------------------------------------------------
def test_closed_loop_coordinated_fleet_ends_no_later(rt):
    """Eight boxers explore the store of examples/fleet_store_frontier.py from one corner (seed 0, at most 3000 control
    steps, a re-plan every 10), once as before (tile = 0: every robot to the nearest frontier cell, the baseline) and
    once coordinated (tile = 8).  Gates on the coordinated run, the conditions of
    test_gpu_exploration.test_closed_loop_fleet_explores_the_store with its constants: exploration ends; at most 0.5 %
    of the free cells are unseen; no seen cell is classified against the truth; at most 1 % failed robot-steps, no base
    centre inside a shelf, the end link at least 0.5 r_body from every shelf; and it ends no later than the baseline run
    beside it.  Measured on the MI355X: the baseline ends at step 200, the coordinated run at step 110,
    both with 1371 of 1371 free cells seen and no failed solve."""
    ex = load_example("fleet_store_frontier")
    base = ex.run(B=8, seed=0, steps=3000, replan_every=10, tile=0)
    r = ex.run(B=8, seed=0, steps=3000, replan_every=10, tile=8)
    print(dict(baseline=base))
    print(dict(coordinated=r))
    assert r["fused"] and set(r) == set(base)
    assert r["ended_step"] is not None and r["frontier_cells"] == 0, r
    assert r["free_cells"] - r["free_cells_seen"] <= 0.005 * r["free_cells"], r
    assert r["map_wrong_cells"] == 0, r
    assert r["failed_share"] <= 0.01, r
    assert r["base_inside"] == 0 and r["min_base_clearance_m"] > 0.0, r
    assert r["min_ee_clearance_m"] >= 0.5 * r["r_body"], r
    base_end = base["ended_step"] if base["ended_step"] is not None else base["steps"]   # a baseline that never ends
    assert r["ended_step"] <= base_end, (r["ended_step"], base["ended_step"])
