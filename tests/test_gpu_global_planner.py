"""The global planner on the device (rmpc_grid_*_device, rmpc_follow_path_device) against the CPU restatement of the
reference's rules in tests/global_planner_reference.py: enlarged obstacles, cost-to-go fields (bitwise on binary maps),
paths, the batched planner, the mirror of the reference's API, the waypoint follower and a closed loop."""
import math

import numpy as np
import pytest

from example_loader import load_example
from global_planner_reference import LocalGoalRef, astar_ref, descend_ref, field_ref, inflate_ref, path_cost
from gpu_support import DEV, _t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import torch
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return dict(torch=torch, lib=_lib)


def _inflated_shelves(rt, H, W, seed, cell=0.45):
    from robot_mpcs_amd.global_planner import shelf_map
    torch = rt["torch"]
    big = H >= 100
    raw = _t(torch, shelf_map(H, W, seed=seed, aisle=9 if big else 4, shelf=4 if big else 2, gap=6 if big else 3))
    out = torch.empty_like(raw)
    rt["lib"].grid_inflate_device(raw, out, cell, 0.45, 0.29)
    return out.cpu().numpy()


def _fields(rt, data, goals, movement):
    torch = rt["torch"]
    G = len(goals)
    H, W = data.shape
    f = torch.full((G, H, W), float("nan"), dtype=torch.float64, device=DEV)
    st = torch.full((G,), 99, dtype=torch.int32, device=DEV)
    sw = torch.zeros(G, dtype=torch.int32, device=DEV)
    rt["lib"].grid_fields_device(_t(torch, data), _t(torch, goals, torch.int32), f, st, movement, sweeps=sw)
    torch.cuda.synchronize()
    return f.cpu().numpy(), st.cpu().numpy(), sw.cpu().numpy()


@pytest.mark.parametrize("H,W,size", [(41, 41, 0.45), (97, 61, 0.9), (128, 128, 0.3)])
def test_inflation_matches_restatement(rt, H, W, size):
    torch = rt["torch"]
    rng = np.random.default_rng(H)
    for data in (rng.uniform(size=(H, W)) ** 3, (rng.uniform(size=(H, W)) < 0.2).astype(float)):
        out = torch.full((H, W), float("nan"), dtype=torch.float64, device=DEV)
        rt["lib"].grid_inflate_device(_t(torch, data), out, 0.45, size, 0.29)
        torch.cuda.synchronize()
        ref, conv = inflate_ref(data, 0.45, size, 0.29)
        differ = out.cpu().numpy() != ref
        assert np.all(np.abs(conv[differ] - 0.29) <= 1e-12)


@pytest.mark.parametrize("movement", [8, 4])
@pytest.mark.parametrize("H,W", [(41, 41), (97, 61), (128, 128)])
def test_fields_equal_cpu_dijkstra(rt, H, W, movement):
    rng = np.random.default_rng(H * W + movement)
    binary = _inflated_shelves(rt, H, W, seed=2)
    graded = np.where(binary > 0.5, 1.0, rng.uniform(0.0, 0.7, size=(H, W)))
    free = np.flatnonzero(binary.ravel() < 0.8)
    for G in (1, 16, 64):
        goals = rng.choice(free, G, replace=False).astype(np.int32)
        check = range(G) if H * W <= 41 * 41 else rng.choice(G, min(G, 3), replace=False)
        for data, exact in ((binary, True), (graded, False)):
            f, st, sw = _fields(rt, data, goals, movement)
            assert np.all(st == 0) and np.all(sw > 0)
            for k in check:
                ref = field_ref(data, int(goals[k]), movement)
                fin = np.isfinite(ref)
                assert np.array_equal(np.isfinite(f[k]), fin)
                if exact:
                    assert np.array_equal(f[k], ref)
                else:
                    assert np.allclose(f[k][fin], ref[fin], rtol=1e-12, atol=0)
            f2, _, _ = _fields(rt, data, goals, movement)
            assert np.array_equal(f, f2)   # run to run


def test_field_status_codes_and_size_limit(rt):
    torch = rt["torch"]
    data = _inflated_shelves(rt, 41, 41, seed=1)
    occ = int(np.flatnonzero(data.ravel() > 0.5)[0])
    f, st, _ = _fields(rt, data, np.array([occ, -1, 41 * 41, int(np.flatnonzero(data.ravel() < 0.5)[0])], np.int32), 8)
    assert list(st) == [-2, -3, -3, 0] and np.all(np.isinf(f[:3]))
    big = torch.zeros((129, 128), dtype=torch.float64, device=DEV)
    with pytest.raises(rt["lib"].RmpcError, match="RMPC_GRID_MAX_CELLS"):
        rt["lib"].grid_fields_device(big, _t(torch, [0], torch.int32), torch.empty((1, 129, 128), dtype=torch.float64, device=DEV),
                                     torch.empty(1, dtype=torch.int32, device=DEV))


def test_field_refuses_negative_free_cells(rt):
    """A free cell with a negative value (e.g. -1 for 'unknown') would give negative prices: the field reports
    RMPC_GRID_BAD_MAP instead of sweeping."""
    data = np.zeros((20, 30))
    data[5, 7] = -1.0
    f, st, sw = _fields(rt, data, np.array([0, 31], np.int32), 8)
    assert list(st) == [rt["lib"].GRID_BAD_MAP] * 2 and np.all(np.isinf(f)) and np.all(sw == 0)
    data[5, 7] = 0.0
    _, st, _ = _fields(rt, data, np.array([0, 31], np.int32), 8)
    assert list(st) == [0, 0]


def test_get_enlarged_obstacles_matches_the_reference_png_path(rt, tmp_path):
    """GlobalPlanner.get_occupancy_map + get_enlarged_obstacles on a 3-D occupancy map equal the reference's own path:
    plt.imsave of the clipped 2-D map, OccupancyGridMap.from_png, then the blur-and-threshold restated."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from robot_mpcs_amd.global_planner import GlobalPlanner, OccupancyGridMap
    rng = np.random.default_rng(21)
    low, high = np.array([-5.0, -5.0, 0.0]), np.array([10.0, 10.0, 0.8])
    for size_robot in (0.4, 0.8):
        occ3d = (rng.uniform(size=(41, 41, 5)) < 0.03).astype(float)
        gp = GlobalPlanner(dim_pixels=np.array([40, 40, 5]), limits_low=low, limits_high=high, BOOL_PLOTTING=False)
        assert gp.get_occupancy_map("sensor", occ3d) == "sensor"
        got = gp.get_enlarged_obstacles(size_robot)
        plt.imsave(tmp_path / "occupancy_map.png", np.clip(np.sum(occ3d, axis=2), 0, gp.threshold))
        ref_map = OccupancyGridMap.from_png(str(tmp_path / "occupancy_map.png"), cell_size=gp.cell_size).data
        ref, conv = inflate_ref(ref_map, gp.cell_size, size_robot, gp.threshold)
        differ = got != ref
        assert np.all(np.abs(conv[differ] - gp.threshold) <= 1e-12) and differ.sum() == 0


def _is_valid_path(data, cells, start, goal, movement):
    H, W = data.shape
    if cells[0] != start or cells[-1] != goal:
        return False
    for a, b in zip(cells[:-1], cells[1:]):
        (ar, ac), (br, bc) = divmod(int(a), W), divmod(int(b), W)
        if max(abs(ar - br), abs(ac - bc)) != 1 or (movement == 4 and abs(ar - br) + abs(ac - bc) != 1):
            return False
    return all(0 <= c < H * W and data.ravel()[c] < 0.8 for c in cells)


@pytest.mark.parametrize("movement", [8, 4])
def test_paths_are_valid_and_optimal(rt, movement):
    from robot_mpcs_amd.global_planner import plan_batch
    torch = rt["torch"]
    rng = np.random.default_rng(movement)
    binary = _inflated_shelves(rt, 41, 41, seed=5)
    graded = np.where(binary > 0.5, 1.0, rng.uniform(0.0, 0.7, size=binary.shape))
    free = np.flatnonzero(binary.ravel() < 0.8)
    B = 48
    starts, goals = rng.choice(free, B).astype(np.int32), rng.choice(free, 6)[rng.integers(0, 6, B)].astype(np.int32)
    for data, exact in ((binary, True), (graded, False)):
        paths, lens, (fields, status, gi) = plan_batch(_t(torch, data), starts, goals, movement=movement, return_fields=True)
        paths, lens, fields, gi = paths.cpu().numpy(), lens.cpu().numpy(), fields.cpu().numpy(), gi.cpu().numpy()
        for b in range(B):
            cells = paths[b, :lens[b]]
            assert lens[b] > 0 and _is_valid_path(data, cells, starts[b], goals[b], movement)
            W = data.shape[1]
            _, acost = astar_ref(data, (starts[b] % W, starts[b] // W), (goals[b] % W, goals[b] // W), movement)
            cost, D = path_cost(data, cells), fields[gi[b]].ravel()[starts[b]]
            assert cost == pytest.approx(D, rel=1e-12, abs=1e-12)
            if exact:
                assert cost == pytest.approx(acost, rel=1e-12, abs=1e-12)
            else:
                assert cost <= acost + 1e-9


def test_path_error_codes(rt):
    from robot_mpcs_amd.global_planner import plan_batch
    torch = rt["torch"]
    lib = rt["lib"]
    data = np.zeros((9, 9))
    data[4, :] = 1.0          # a wall: the lower half cannot reach the upper
    data[0, 0] = 1.0
    W = 9
    # start occupied, goal occupied, start outside, unreachable, too long (max_len 3), fine
    starts = np.array([0, 10, -5, 10, 10, 10], np.int32)
    goals = np.array([11, 0, 11, 70, 35, 12], np.int32)
    paths, lens = plan_batch(_t(torch, data), starts, goals, max_len=3)
    lens = lens.cpu().numpy()
    assert list(lens[:5]) == [lib.GRID_START_OCCUPIED, lib.GRID_GOAL_OCCUPIED, lib.GRID_OUTSIDE, 0, lib.GRID_TOO_LONG]
    assert lens[5] == 3 and list(paths[5, :3].cpu().numpy()) == [10, 11, 12]
    # a goal index outside [0, G)
    fields = torch.zeros((1, 9, 9), dtype=torch.float64, device=DEV)
    path = torch.empty((1, 4), dtype=torch.int32, device=DEV)
    ln = torch.empty(1, dtype=torch.int32, device=DEV)
    lib.grid_paths_device(_t(torch, data), fields, _t(torch, [12], torch.int32), _t(torch, [10], torch.int32),
                          _t(torch, [1], torch.int32), path, ln)
    assert int(ln.item()) == lib.GRID_OUTSIDE
    with pytest.raises(ValueError):
        plan_batch(_t(torch, data), starts, goals, movement="6N")


def test_4096_queries_on_a_128_map_match_per_query_cpu_runs(rt):
    from robot_mpcs_amd.global_planner import plan_batch
    torch = rt["torch"]
    rng = np.random.default_rng(7)
    data = _inflated_shelves(rt, 128, 128, seed=3)
    free = np.flatnonzero(data.ravel() < 0.8)
    goal_set = rng.choice(free, 16, replace=False)
    B = 4096
    starts, goals = rng.choice(free, B).astype(np.int32), goal_set[rng.integers(0, 16, B)].astype(np.int32)
    p1, l1 = plan_batch(_t(torch, data), starts, goals)
    p2, l2 = plan_batch(_t(torch, data), starts, goals)
    p1, l1, p2, l2 = p1.cpu().numpy(), l1.cpu().numpy(), p2.cpu().numpy(), l2.cpu().numpy()
    assert np.array_equal(l1, l2) and all(np.array_equal(p1[b, :l1[b]], p2[b, :l2[b]]) for b in range(B))
    ref_fields = {int(g): field_ref(data, int(g)) for g in goal_set}
    for b in range(B):
        D = ref_fields[int(goals[b])]
        assert l1[b] > 0
        assert list(p1[b, :l1[b]]) == descend_ref(data, D, int(starts[b]), int(goals[b]))


def test_a_star_and_global_planner_mirror(rt):
    from robot_mpcs_amd.global_planner import GlobalPlanner, OccupancyGridMap, a_star, shelf_map
    rng = np.random.default_rng(4)
    raw = shelf_map(41, 41, seed=6)
    data = _inflated_shelves(rt, 41, 41, seed=6, cell=0.375)
    gmap = OccupancyGridMap(data.copy(), 0.375)
    free = np.flatnonzero(data.ravel() < 0.8)
    for _ in range(10):
        s, g = rng.choice(free, 2, replace=False)
        sm, gm = ((s % 41) * 0.375, (s // 41) * 0.375), ((g % 41) * 0.375, (g // 41) * 0.375)
        path, path_idx = a_star(sm, gm, gmap)
        ref_idx, ref_cost = astar_ref(data, (s % 41, s // 41), (g % 41, g // 41))
        assert isinstance(path, list) and isinstance(path_idx, list) and isinstance(path_idx[0], tuple)
        assert path_idx[0] == ref_idx[0] and path_idx[-1] == ref_idx[-1]
        assert path == [(x * 0.375, y * 0.375) for x, y in path_idx]
        assert path_cost(data, [y * 41 + x for x, y in path_idx]) == pytest.approx(ref_cost, rel=1e-12)
    occ = np.flatnonzero(data.ravel() > 0.5)[0]
    with pytest.raises(Exception, match="Start node is not traversable"):
        a_star(((occ % 41) * 0.375, (occ // 41) * 0.375), (0.375 * (free[0] % 41), 0.375 * (free[0] // 41)), gmap)
    with pytest.raises(Exception, match="outside"):
        a_star((-5.0, 0.0), (1.0, 1.0), gmap)

    # the reference's example setup: a 41-cell sensor over [-5, 10] m, the map given in the planner's image frame
    low, high = np.array([-5.0, -5.0, 0.0]), np.array([10.0, 10.0, 0.8])
    gp = GlobalPlanner(dim_pixels=np.array([40, 40, 5]), limits_low=low, limits_high=high, BOOL_PLOTTING=False)
    gp.set_occupancy_map(raw)
    enlarged = gp.get_enlarged_obstacles()
    assert np.array_equal(enlarged, inflate_ref(raw, gp.cell_size, 0.4, 0.29)[0])
    for _ in range(5):
        s, g = rng.choice(np.flatnonzero(enlarged.ravel() < 0.8), 2, replace=False)
        start = gp.convert_meters_reversed(((s % 41) * gp.cell_size, (s // 41) * gp.cell_size))
        goal = gp.convert_meters_reversed(((g % 41) * gp.cell_size, (g // 41) * gp.cell_size))
        wpath, px = gp.get_global_path_astar(start, goal)
        ref_idx, ref_cost = astar_ref(enlarged, (s % 41, s // 41), (g % 41, g // 41))
        if not ref_idx:
            assert wpath == [] and px == []
            continue
        assert px[0] == ref_idx[0] and px[-1] == ref_idx[-1]
        assert path_cost(enlarged, [y * 41 + x for x, y in px]) == pytest.approx(ref_cost, rel=1e-12)
        assert len(wpath) == len(px) and all(len(w) == 3 for w in wpath)
        assert np.allclose(wpath[0][:2], start[:2], atol=1e-9) and np.allclose(wpath[-1][:2], goal[:2], atol=1e-9)
        lg = GlobalPlanner(np.array([40, 40, 5]), low, high, BOOL_PLOTTING=False)
        ref = LocalGoalRef(1.3)
        for p in wpath[::2]:
            assert np.array_equal(lg.get_local_goal(p[:2], wpath), ref(p[:2], wpath))


def test_route_follower_matches_local_goal_restatement(rt):
    from robot_mpcs_amd.global_planner import RouteFollower, cells_from_positions, plan_batch, shelf_map
    torch = rt["torch"]
    rng = np.random.default_rng(12)
    H = W = 41
    cell, x0, y0 = 0.45, -9.0, -9.0
    data = _inflated_shelves(rt, H, W, seed=8)
    free = np.flatnonzero(data.ravel() < 0.8)
    B, T = 64, 120
    starts, goals = rng.choice(free, B).astype(np.int32), rng.choice(free, B).astype(np.int32)
    paths, lens = plan_batch(_t(torch, data), starts, goals)
    f = RouteFollower(paths, lens, W, x0, y0, cell, threshold=1.3)
    P, L = paths.cpu().numpy(), lens.cpu().numpy()
    world = [[(x0 + (c % W) * cell, y0 + (c // W) * cell) for c in P[b, :L[b]]] for b in range(B)]
    # recorded positions: a noisy walk along each route, sometimes stalling
    pos = np.zeros((T, B, 6))
    for b in range(B):
        k = np.minimum(np.cumsum(rng.integers(0, 3, T)), L[b] - 1)
        pos[:, b, :2] = np.array(world[b])[k] + rng.normal(0, 0.4, (T, 2))
    refs = [LocalGoalRef(1.3) for _ in range(B)]
    goal = torch.full((B, 3), float("nan"), dtype=torch.float64, device=DEV)
    for t in range(T):
        x = _t(torch, pos[t])
        f.step(x, goal)
        got_idx, got_goal = f.idx.cpu().numpy(), goal.cpu().numpy()
        for b in range(B):
            want = refs[b](pos[t, b, :2], world[b])
            assert got_idx[b] == refs[b].idx
            assert got_goal[b, 0] == want[0] and got_goal[b, 1] == want[1] and got_goal[b, 2] == 0.0
    # world positions -> cells (xinit as it is, stride 6)
    cells = cells_from_positions(_t(torch, pos[-1]), H, W, x0, y0, cell).cpu().numpy()
    col, row = np.rint((pos[-1, :, 0] - x0) / cell), np.rint((pos[-1, :, 1] - y0) / cell)
    inside = (col >= 0) & (col < W) & (row >= 0) & (row < H)
    assert np.array_equal(cells, np.where(inside, row * W + col, -1).astype(np.int32))


def test_closed_loop_reaches_final_goals_across_shelves(rt):
    """256 point robots (cfg2 model) on a 41 x 41 shelf map (0.45 m cells) enlarged as the reference does it, final
    goals 10 .. 20 m away behind a shelf, follow -> solve_scene_device -> advance_device on the device
    (examples/fleet_global_route.py, defaults, seed 0).  First MI355X measurement over 1200 control steps: all 256
    routes found, 0 failed solves, all 256 robots within ARRIVE_TOL (0.25 m) of their final goal by control step 311
    (p50 195, p90 258), least clearance between a robot's centre and a raw-occupied cell 0.036 m (p10 0.092 m).
    Gate: no failed solve, clearance > 0 throughout, SHARE = 0.9 of the robots arrived by STEPS = 420 (35 % more
    steps than the last arrival)."""
    SHARE, STEPS = 0.9, 420
    ex = load_example("fleet_global_route")
    r = ex.run(B=256, steps=STEPS, seed=0)
    assert r["routes"] == 256
    assert r["failed_solves"] == 0
    assert r["min_clearance_m"] > 0.0, r
    assert r["arrival_share"] >= SHARE, r
