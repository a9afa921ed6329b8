"""Traffic-aware routes on the device (include/rmpc_traffic.h) against the restatement of
tests/traffic_reference.py, equality of all bits: the flow table after adding and removing routes at the sizes where the
launch's blocks switch; the fields on the maps where the field kernel changes its layout (one cell, one row, runs of
one cell, just above 1024 cells, the limit with runs of 17), both movements, on tables that are empty, below the caps,
above them and negative, into outputs prefilled with a sentinel; the descents with every value ``d_len`` can take; the
score; the refusals, which must leave the outputs alone; ``TrafficRoutes.plan`` and ``replan`` against the restated
loop and against the calls made by hand; one small closed loop of the store example."""
import numpy as np
import pytest

from example_loader import load_example
from gpu_support import DEV, _t
from traffic_cases import COSTS, FLOWS, OCC, SIZES, UNIT, field_map, flow_table, fleet_case, goal_list, serpentine_map
from traffic_reference import (GOAL_OCCUPIED, INF, MOVES, OK, OUTSIDE, START_OCCUPIED, TOO_LONG, add_ref, count_routes, descend_ref,
                               field_heap, field_ref, free_cells, plan_ref, route_cost, score_ref)

pytestmark = pytest.mark.gpu

FILL = -9
REFS = {}


@pytest.fixture(scope="module")
def rt():
    import torch
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.global_planner import RouteFollower, TrafficRoutes
    return dict(torch=torch, lib=_lib, TrafficRoutes=TrafficRoutes, RouteFollower=RouteFollower)


def i32(rt, a):
    return _t(rt["torch"], a, rt["torch"].int32)


def filled(rt, shape, dtype=None):
    torch = rt["torch"]
    return torch.full(shape, FILL, dtype=dtype or torch.int32, device=DEV)


def once(key, make):
    """a reference computed once per key and left unchanged"""
    if key not in REFS:
        REFS[key] = make()
    return REFS[key]


# ---- the flow table ---------------------------------------------------------------------------------------------------
def route_batch(B, max_len, H, W, seed=0):
    """B rows of every kind the header names: walks by single moves, with repeated cells, jumps, cells outside the map;
    lengths that are negative, 0, up to max_len and beyond it"""
    rng = np.random.default_rng([seed, B, max_len])
    paths = np.zeros((B, max_len), np.int32)
    for b in range(B):
        r, c = int(rng.integers(0, H)), int(rng.integers(0, W))
        for j in range(max_len):
            paths[b, j] = r * W + c
            kind = rng.random()
            if kind < 0.75:                                             # one move, inside the map (else the cell repeats)
                dc, dr = MOVES[int(rng.integers(0, 8))]
                if 0 <= r + dr < H and 0 <= c + dc < W:
                    r, c = r + dr, c + dc
            elif kind < 0.85:                                           # a jump
                r, c = int(rng.integers(0, H)), int(rng.integers(0, W))
        out = rng.random(max_len) < 0.05
        paths[b, out] = rng.choice([-1, -7, H * W, H * W + 5, 2 ** 31 - 1], int(out.sum()))
    lens = rng.integers(-2, max_len + 3, B).astype(np.int32)
    lens[rng.random(B) < 0.1] = max_len
    return paths, lens


@pytest.mark.parametrize("B,max_len", [(1, 40), (63, 40), (64, 40), (65, 40), (257, 40), (65, 1)])
def test_add_and_remove_equal_the_restatement(rt, B, max_len):
    lib, (H, W) = rt["lib"], (25, 41)
    paths, lens = route_batch(B, max_len, H, W)
    select = (np.random.default_rng(B).random(B) < 0.6).astype(np.int32) * 3
    start = flow_table("negative", H, W)
    for sel in (None, select):
        want = once(("add", B, max_len, sel is None), lambda: add_ref(start.copy(), paths, lens, 1, sel))
        flow = i32(rt, start)
        lib.grid_traffic_add_device(flow, i32(rt, paths), i32(rt, lens), 1, select=None if sel is None else i32(rt, sel))
        got = flow.cpu().numpy()
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
        lib.grid_traffic_add_device(flow, i32(rt, paths), i32(rt, lens), -1, select=None if sel is None else i32(rt, sel))
        assert np.array_equal(flow.cpu().numpy(), start)               # add then remove: the prefilled table is back


def test_4096_copies_of_one_route_count_4096(rt):
    lib, torch = rt["lib"], rt["torch"]
    route = [0, 1, 43, 44, 44, 85, 2]                                   # 41 wide: +col, (+1, +1), +col, a stop, +row, a jump
    paths = np.tile(np.array(route + [7] * 3, np.int32), (4096, 1))
    flow = torch.zeros((9, 5, 41), dtype=torch.int32, device=DEV)
    lib.grid_traffic_add_device(flow, i32(rt, paths), i32(rt, np.full(4096, len(route), np.int32)))
    got = flow.cpu().numpy()
    want = 4096 * count_routes(5, 41, [route])
    assert np.array_equal(got, want) and got[8].ravel()[44] == 8192 and got[0].ravel()[[0, 43]].tolist() == [4096, 4096]
    assert got[4].ravel()[1] == 4096 and got[1].ravel()[44] == 4096 and got[:8].sum() == 4 * 4096 and got[8].sum() == 7 * 4096


# ---- the fields -------------------------------------------------------------------------------------------------------
def device_fields(rt, grid, flow, k, goals, movement, sweeps=True):
    lib = rt["lib"]
    G, (H, W) = len(goals), grid.shape
    fields, status = filled(rt, (G, H, W)), filled(rt, (G,))
    sw = filled(rt, (G,)) if sweeps else None
    lib.grid_fields_traffic_device(_t(rt["torch"], grid), i32(rt, flow), lib.traffic_costs(**k), i32(rt, goals), fields, status,
                                   movement, OCC, sweeps=sw)
    return fields.cpu().numpy(), status.cpu().numpy(), None if sw is None else sw.cpu().numpy()


def reference_fields(size, kind, movement, goals, k=COSTS, name="COSTS"):
    grid, flow = field_map(*size), flow_table(kind, *size)
    return once(("fields", size, kind, movement, len(goals), name),
                lambda: [field_ref(grid, OCC, flow, k, int(g), movement) for g in goals])


def check_fields(got, want, H, W):
    fields, status, sweeps = got
    assert status.tolist() == [s for _, s in want]
    for g, (D, s) in enumerate(want):
        assert np.array_equal(fields[g], D), (g, np.argwhere(fields[g] != D)[:5])
        if s != OK:
            assert (fields[g] == INF).all()
        if sweeps is not None:
            assert (1 <= sweeps[g] <= H * W + 1) if s == OK else sweeps[g] == 0


@pytest.mark.parametrize("movement", [4, 8])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_one_field_on_every_size_and_table(rt, size, movement):
    grid = field_map(*size)
    goals = goal_list(grid, 1)
    for kind in FLOWS:
        want = reference_fields(size, kind, movement, goals)
        got = device_fields(rt, grid, flow_table(kind, *size), COSTS, goals, movement, sweeps=kind != "below")
        check_fields(got, want, *size)
    assert want[0][1] == OK and (size == (1, 1) or (want[0][0] < INF).sum() > 1)
    if size[0] * size[1] >= 37:
        assert (want[0][0][free_cells(grid, OCC)] == INF).any()         # a free region no route leads from


@pytest.mark.parametrize("movement", [4, 8])
@pytest.mark.parametrize("kind", FLOWS)
@pytest.mark.parametrize("size", [(25, 41), (41, 41)], ids=["25x41", "41x41"])
def test_seventy_fields_with_occupied_and_outside_goals(rt, size, kind, movement):
    grid = field_map(*size)
    goals = goal_list(grid, 70)
    want = reference_fields(size, kind, movement, goals)
    assert sorted({s for _, s in want}) == [OUTSIDE, GOAL_OCCUPIED, OK] and [s for _, s in want].count(OUTSIDE) == 2
    check_fields(device_fields(rt, grid, flow_table(kind, *size), COSTS, goals, movement), want, *size)


def test_field_equals_the_heap_dijkstra_at_the_limit(rt):
    size = (128, 128)
    grid, flow = field_map(*size), flow_table("below", *size)
    goals = goal_list(grid, 1)
    want = once(("heap", size), lambda: field_heap(grid, OCC, flow, COSTS, int(goals[0]), 8))
    got = device_fields(rt, grid, flow, COSTS, goals, 8)
    assert np.array_equal(got[0][0], want[0]) and got[1][0] == OK and (want[0] < INF).sum() > 8000


@pytest.mark.parametrize("movement", [4, 8])
@pytest.mark.parametrize("size", [(41, 41), (128, 128)], ids=["41x41", "128x128"])
def test_field_along_one_lane_through_the_whole_map(rt, size, movement):
    """the deepest shortest-path tree a map of the size has: the far end is about H / 2 rows of W cells away.  A sweep
    carries a value at most two runs of a thread's cells further (2 x 3 cells at 41 x 41, 2 x 17 at 128 x 128), so the
    field takes more than H sweeps, where the store's takes about H.  The heap Dijkstra is the reference; the second
    goal is the map's last cell, free at 41 x 41 and a wall at 128 x 128."""
    grid, flow = serpentine_map(*size), flow_table("below", *size)
    goals = np.array([0, size[0] * size[1] - 1], np.int32)
    want = once(("lane", size, movement), lambda: [field_heap(grid, OCC, flow, COSTS, int(g), movement) for g in goals])
    got = device_fields(rt, grid, flow, COSTS, goals, movement)
    check_fields(got, want, *size)
    free = free_cells(grid, OCC)
    assert (want[0][0][free] < INF).all() and got[2][0] > size[0]


# ---- the descents -----------------------------------------------------------------------------------------------------
def path_case(B, movement):
    size = (41, 41)
    grid, flow = field_map(*size), flow_table("below", *size)
    goals = goal_list(grid, 8)
    rng = np.random.default_rng([B, movement])
    starts = rng.integers(0, 41 * 41, B).astype(np.int32)              # free and occupied cells alike
    index = rng.integers(0, 8, B).astype(np.int32)
    starts[::5] = rng.choice(np.flatnonzero(free_cells(grid, OCC).ravel()), len(starts[::5]))
    if B > 8:
        starts[1], starts[2], index[3], index[4] = -1, 41 * 41, -1, 8
        index[5], starts[5] = 0, goals[0]                               # start equal to the goal
        starts[6], index[6] = 3 * 41 + 3, 0                             # inside the walled box: no route
    return grid, flow, goals, starts, index


def device_paths(rt, grid, flow, k, fields, goals, starts, index, movement, max_len):
    lib = rt["lib"]
    path, length = filled(rt, (len(starts), max_len)), filled(rt, (len(starts),))
    lib.grid_paths_traffic_device(_t(rt["torch"], grid), i32(rt, flow), lib.traffic_costs(**k), i32(rt, fields), i32(rt, goals),
                                  i32(rt, starts), i32(rt, index), path, length, movement, OCC)
    return path.cpu().numpy(), length.cpu().numpy()


def check_paths(got, want, max_len):
    path, length = got
    assert length.tolist() == [n for _, n in want]
    for b, (cells, n) in enumerate(want):
        if n > 0:
            assert path[b, :n].tolist() == cells and (path[b, n:] == FILL).all()
        elif n != TOO_LONG:
            assert (path[b] == FILL).all()


MAX_LEN = 4 * 82


def reference_paths(B, movement):
    grid, flow, goals, starts, index = path_case(B, movement)
    fields = np.stack([D for D, _ in reference_fields((41, 41), "below", movement, goals)])
    max_len = MAX_LEN

    def make():
        out = []
        for s, gi in zip(starts, index):
            if not 0 <= gi < 8:
                out.append(([], OUTSIDE))
            else:
                out.append(descend_ref(grid, OCC, flow, COSTS, fields[gi], int(s), int(goals[gi]), movement, max_len))
        return out

    return fields, once(("paths", B, movement), make)


@pytest.mark.parametrize("movement", [4, 8])
@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_descents_equal_the_restatement(rt, B, movement):
    grid, flow, goals, starts, index = path_case(B, movement)
    fields, want = reference_paths(B, movement)
    max_len = MAX_LEN
    check_paths(device_paths(rt, grid, flow, COSTS, fields, goals, starts, index, movement, max_len), want, max_len)
    if B > 8:
        seen = {n for _, n in want if n <= 0}
        assert {0, START_OCCUPIED, GOAL_OCCUPIED, OUTSIDE} <= seen and want[5] == ([int(goals[0])], 1) and want[6][1] == 0
        assert max(n for _, n in want) > 20


def test_a_max_len_one_short_is_too_long(rt):
    grid, flow, goals, starts, index = path_case(257, 8)
    fields, want = reference_paths(257, 8)
    b = int(np.argmax([n for _, n in want]))
    cells, n = want[b]
    assert n > 20
    for max_len, length in ((n, n), (n - 1, TOO_LONG)):
        path, got = device_paths(rt, grid, flow, COSTS, fields, goals, starts[b:b + 1], index[b:b + 1], 8, max_len)
        assert got.tolist() == [length] and path[0].tolist() == cells[:max_len]
        assert descend_ref(grid, OCC, flow, COSTS, fields[index[b]], int(starts[b]), int(goals[index[b]]), 8, max_len)[1] == length


def test_zero_weights_are_the_global_planners_fields_and_routes(rt):
    """movement 4, base 1, no weights: the values of rmpc_grid_fields_device at cost factor 0 (integers in doubles) and
    the routes of rmpc_grid_paths_device, whatever the table holds"""
    torch, lib = rt["torch"], rt["lib"]
    grid, starts, goals = fleet_case(B=257, H=41, W=41)
    uniq, index = np.unique(goals, return_inverse=True)
    flow = flow_table("above", 41, 41)
    got = device_fields(rt, grid, flow, UNIT, uniq.astype(np.int32), 4)
    g = _t(torch, grid)
    fields, status = torch.empty((len(uniq), 41, 41), dtype=torch.float64, device=DEV), filled(rt, (len(uniq),))
    lib.grid_fields_device(g, i32(rt, uniq), fields, status, 4, OCC, 0.0)
    want = fields.cpu().numpy()
    assert (got[1] == OK).all() and (status.cpu().numpy() == OK).all()
    assert np.array_equal(np.where(got[0] == INF, np.inf, got[0].astype(np.float64)), want)
    path, length = filled(rt, (257, 164)), filled(rt, (257,))
    lib.grid_paths_device(g, fields, i32(rt, uniq), i32(rt, starts), i32(rt, index), path, length, 4, OCC, 0.0)
    mine = device_paths(rt, grid, flow, UNIT, got[0], uniq.astype(np.int32), starts, index.astype(np.int32), 4, 164)
    assert np.array_equal(mine[1], length.cpu().numpy()) and (mine[1] > 1).all() and np.array_equal(mine[0], path.cpu().numpy())


# ---- the score --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FLOWS)
@pytest.mark.parametrize("size", [(1, 1), (1, 37), (25, 41), (128, 128)], ids=["1x1", "1x37", "25x41", "128x128"])
def test_score_equals_numpy(rt, size, kind):
    torch, lib = rt["torch"], rt["lib"]
    flow = flow_table(kind, *size)
    score = filled(rt, (3,), torch.int64)
    lib.grid_traffic_score_device(i32(rt, flow), score, 1000, 1414)
    assert tuple(score.cpu().tolist()) == score_ref(flow, 1000, 1414)
    lib.grid_traffic_score_device(i32(rt, flow), score, 3, 1)
    assert tuple(score.cpu().tolist()) == score_ref(flow, 3, 1)


# ---- the refusals leave the outputs alone ---------------------------------------------------------------------------------
def test_refused_calls_write_nothing(rt):
    torch, lib = rt["torch"], rt["lib"]
    from robot_mpcs_amd._abi import RmpcError
    grid, flow = _t(torch, field_map(25, 41)), i32(rt, flow_table("below", 25, 41))
    goals, starts, index = i32(rt, [100, 200]), i32(rt, [50, 60, 70]), i32(rt, [0, 1, 0])
    fields, status, sweeps = filled(rt, (2, 25, 41)), filled(rt, (2,)), filled(rt, (2,))
    path, length, score = filled(rt, (3, 30)), filled(rt, (3,)), filled(rt, (3,), torch.int64)
    bad_costs = [dict(base_axial=0), dict(base_diag=-1), dict(w_visit=-1), dict(cap_visit=-1), dict(w_contra=-1), dict(cap_contra=-1),
                 dict(cap_visit=256), dict(cap_contra=16), dict(w_visit=2000), dict(base_axial=65536)]
    for bad in bad_costs:
        with pytest.raises(RmpcError, match="grid fields traffic"):
            lib.grid_fields_traffic_device(grid, flow, lib.traffic_costs(**bad), goals, fields, status, 8, OCC, sweeps=sweeps)
        with pytest.raises(RmpcError, match="grid paths traffic"):
            lib.grid_paths_traffic_device(grid, flow, lib.traffic_costs(**bad), fields, goals, starts, index, path, length, 8, OCC)
    for movement in (0, 6):
        with pytest.raises(RmpcError, match="movement must be 4 or 8"):
            lib.grid_fields_traffic_device(grid, flow, lib.traffic_costs(), goals, fields, status, movement, OCC, sweeps=sweeps)
        with pytest.raises(RmpcError, match="movement must be 4 or 8"):
            lib.grid_paths_traffic_device(grid, flow, lib.traffic_costs(), fields, goals, starts, index, path, length, movement, OCC)
    table = i32(rt, flow_table("below", 25, 41))
    for sign in (0, 2, -3):
        with pytest.raises(RmpcError, match="sign must be"):
            lib.grid_traffic_add_device(table, i32(rt, np.full((3, 30), 5)), i32(rt, [30, 30, 30]), sign)
    for bases in ((0, 1), (1, 0)):
        with pytest.raises(RmpcError, match="base_axial and base_diag"):
            lib.grid_traffic_score_device(flow, score, *bases)
    # a map above the limit: 129 x 128
    big, big_flow = torch.zeros((129, 128), dtype=torch.float64, device=DEV), torch.full((9, 129, 128), FILL, dtype=torch.int32, device=DEV)
    big_fields = filled(rt, (2, 129, 128))
    with pytest.raises(RmpcError, match="129x128 map exceeds RMPC_GRID_MAX_CELLS"):
        lib.grid_fields_traffic_device(big, big_flow, lib.traffic_costs(), goals, big_fields, status, 8, OCC, sweeps=sweeps)
    with pytest.raises(RmpcError, match="129x128 map exceeds RMPC_GRID_MAX_CELLS"):
        lib.grid_paths_traffic_device(big, big_flow, lib.traffic_costs(), big_fields, goals, starts, index, path, length, 8, OCC)
    with pytest.raises(RmpcError, match="129x128 map exceeds RMPC_GRID_MAX_CELLS"):
        lib.grid_traffic_add_device(big_flow, i32(rt, np.full((3, 30), 5)), i32(rt, [30, 30, 30]), 1)
    with pytest.raises(RmpcError, match="129x128 map exceeds RMPC_GRID_MAX_CELLS"):
        lib.grid_traffic_score_device(big_flow, score, 1000, 1414)
    torch.cuda.synchronize()
    for out in (fields, status, sweeps, path, length, score, big_fields, big_flow):
        assert (out == FILL).all()
    assert np.array_equal(table.cpu().numpy(), flow_table("below", 25, 41))


# ---- TrafficRoutes ----------------------------------------------------------------------------------------------------
ROUNDS = 3


def planned(rt, groups, movement="8N"):
    grid, starts, goals = fleet_case()
    tr = rt["TrafficRoutes"](grid, starts, goals, movement=movement, costs=rt["lib"].traffic_costs(**COSTS), groups=groups,
                             rounds=ROUNDS, device=DEV)
    paths, lens = tr.plan()
    assert paths is tr.paths and lens is tr.lens
    return tr


def routes_of(paths, lens):
    return [paths[b, :max(int(n), 0)].tolist() for b, n in enumerate(lens)]


@pytest.mark.parametrize("groups", [1, 5, 24])
def test_plan_equals_the_restated_loop(rt, groups):
    grid, starts, goals = fleet_case()
    want = once(("plan", groups), lambda: plan_ref(grid, OCC, COSTS, starts, goals, 8, groups=groups, rounds=ROUNDS))
    tr = planned(rt, groups)
    lens = tr.lens.cpu().numpy()
    assert np.array_equal(lens, want[1]) and (lens > 1).all() and tr.paths.shape == (24, 4 * 42)
    assert routes_of(tr.paths.cpu().numpy(), lens) == want[0]
    assert np.array_equal(tr.flow.cpu().numpy(), want[2]) and tr.flow.dtype == rt["torch"].int32
    assert np.array_equal(tr.scores.cpu().numpy(), want[3]) and tr.scores.shape == (ROUNDS + 1, 3)
    assert np.array_equal(tr.flow.cpu().numpy(), count_routes(21, 21, want[0]))        # the table invariant, on the device
    tr.plan()                                                           # a second plan starts from the empty table again
    assert np.array_equal(tr.flow.cpu().numpy(), want[2]) and np.array_equal(tr.scores.cpu().numpy(), want[3])


def test_groups_of_one_lower_the_potential_and_end_in_best_responses(rt):
    """J = B on the device's own routes and scores: the potential L + w_visit V + w_contra C never rises from round to
    round and falls overall; the fleet of 24 is at rest after two rounds (tests/test_traffic_cpu.py), so the third
    repeats the second; no cap binds; and every robot's final route costs, under the flow of the others, what the heap
    Dijkstra gives as the least cost from its start: a best response"""
    grid, starts, goals = fleet_case()
    tr = planned(rt, 24)
    scores, flow, lens = tr.scores.cpu().numpy(), tr.flow.cpu().numpy(), tr.lens.cpu().numpy()
    routes = routes_of(tr.paths.cpu().numpy(), lens)
    pot = [int(L) + COSTS["w_visit"] * int(V) + COSTS["w_contra"] * int(Cf) for L, V, Cf in scores]
    assert all(a >= b for a, b in zip(pot[:-1], pot[1:])) and pot[0] > pot[-1]
    assert scores[3].tolist() == scores[2].tolist()
    assert flow.min() >= 0 and flow[8].max() < COSTS["cap_visit"] and flow[:8].max() < COSTS["cap_contra"]
    for b, route in enumerate(routes):
        others = flow - count_routes(21, 21, [route])
        D, _ = field_heap(grid, OCC, others, COSTS, int(goals[b]), 8)
        assert route[0] == starts[b] and route[-1] == goals[b] and len(set(route)) == len(route)
        assert route_cost(others, COSTS, route, 21) == D.flat[starts[b]]


def test_replan_is_cells_plan_and_replace_made_by_hand(rt):
    torch, lib = rt["torch"], rt["lib"]
    grid, starts, goals = fleet_case()
    x0, y0, cell = -3.0, -2.0, 0.5
    tr = planned(rt, 5)
    follower = rt["RouteFollower"](tr.paths.clone(), tr.lens.clone(), 21, x0, y0, cell)
    old_paths, old_lens = tr.paths.cpu().numpy().copy(), tr.lens.cpu().numpy().copy()
    follower.idx += 2
    # every robot stands near the fourth cell of its route (or its last); robot 3 has left the map, robot 4 stands in a shelf
    at = np.array([old_paths[b, min(3, old_lens[b] - 1)] for b in range(24)])
    xy = np.stack([x0 + (at % 21) * cell + 0.1, y0 + (at // 21) * cell - 0.2, np.zeros(24)], 1)
    xy[3, :2] = (x0 - 5.0, y0)
    occupied = np.flatnonzero(~free_cells(grid, OCC).ravel())
    xy[4, :2] = (x0 + (occupied[40] % 21) * cell, y0 + (occupied[40] // 21) * cell)
    xinit = _t(torch, xy)
    paths, lens = tr.replan(follower, xinit)
    cells = filled(rt, (24,))
    lib.grid_cells_device(xinit, cells, 21, 21, x0, y0, cell)
    assert cells.cpu().tolist() == [-1 if b == 3 else int(occupied[40]) if b == 4 else int(at[b]) for b in range(24)]
    assert np.array_equal(tr.starts.cpu().numpy(), cells.cpu().numpy())
    by_hand = rt["TrafficRoutes"](grid, cells, goals, costs=lib.traffic_costs(**COSTS), groups=5, rounds=ROUNDS, device=DEV)
    by_hand.plan()
    new_lens = by_hand.lens.cpu().numpy()
    assert new_lens[3] == OUTSIDE and new_lens[4] == START_OCCUPIED and (np.delete(new_lens, [3, 4]) > 0).all()
    assert np.array_equal(lens.cpu().numpy(), new_lens) and np.array_equal(tr.flow.cpu().numpy(), by_hand.flow.cpu().numpy())
    assert np.array_equal(tr.scores.cpu().numpy(), by_hand.scores.cpu().numpy())
    assert routes_of(paths.cpu().numpy(), new_lens) == routes_of(by_hand.paths.cpu().numpy(), new_lens)
    # the follower: new routes from their first cell; robots 3 and 4 keep their route and their waypoint
    f_paths, f_lens, f_idx = follower.paths.cpu().numpy(), follower.lens.cpu().numpy(), follower.idx.cpu().numpy()
    for b in range(24):
        if b in (3, 4):
            assert f_lens[b] == old_lens[b] and f_idx[b] == 2 and np.array_equal(f_paths[b], old_paths[b])
        else:
            assert f_lens[b] == new_lens[b] and f_idx[b] == 0 and f_paths[b, 0] == at[b]
            assert f_paths[b, :int(new_lens[b])].tolist() == by_hand.paths[b, :int(new_lens[b])].cpu().tolist()


# ---- closed loop -------------------------------------------------------------------------------------------------------
def test_closed_loop_of_the_store_example_on_traffic_aware_routes(rt):
    """16 boxers cross the store (examples/fleet_store_traffic.py, seed 0, 260 steps: the size and step count of the store
    loop in tests/test_gpu_timed.py) on traffic-aware routes.  It runs to the end, every route it followed is a valid
    route on the map (from the robot's start to its goal by single moves over free cells, no cell twice), and the
    reported fields are present.  No gain is asserted (DESIGN.md 30 states what was measured)."""
    ex = load_example("fleet_store_traffic")
    keep = {}
    r = ex.run(B=16, steps=260, seed=0, mode="traffic", keep=keep)
    print(r)
    for field in ("arrivals", "min_pair_gap_m", "failed_solves", "failed_share", "scores_LVC", "plan_ms", "ms_per_step", "routes"):
        assert field in r, field
    assert r["mode"] == "traffic" and r["robots"] == 16 and r["steps"] == 260 and r["routes"] == 16
    assert len(r["scores_LVC"]) == r["rounds"] + 1 and all(len(row) == 3 for row in r["scores_LVC"])
    assert 0 <= r["arrivals"] <= 16 and np.isfinite(r["min_pair_gap_m"]) and 0.0 <= r["failed_share"] <= 1.0
    grid, W = keep["grid"], keep["grid"].shape[1]
    free = free_cells(grid, 0.8).ravel()
    for b in range(16):
        route = keep["paths"][b, :keep["lens"][b]].tolist()
        assert route[0] == keep["starts"][b] and route[-1] == keep["goals"][b] and len(set(route)) == len(route)
        assert free[route].all()
        assert all((v % W - u % W, v // W - u // W) in MOVES for u, v in zip(route[:-1], route[1:]))
    flow = count_routes(*grid.shape, [keep["paths"][b, :keep["lens"][b]].tolist() for b in range(16)])
    assert list(score_ref(flow, 1000, 1414)) == r["scores_LVC"][-1]
