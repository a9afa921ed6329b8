"""The minimum-cost assignment on the device (rmpc_assign_optimal_device, include/rmpc_assign_opt.h)
against the restatement of tests/assign_optimal_reference.py, bit for bit: assign, total, count and steps; several
problems in one call, poisoned buffers, NULL outputs, stream order, the scale; GoalAssigner against the composed
restatements of the planner."""
import math

import numpy as np
import pytest

from assign_optimal_cases import KINDS, make_costs
from assign_optimal_reference import assign_optimal_ref, quantise
from assignment_reference import greedy_ref, route_costs_ref
from global_planner_reference import descend_ref, field_ref
from gpu_support import DEV, _t

pytestmark = pytest.mark.gpu

INF, NAN = math.inf, math.nan
REFS = {}


@pytest.fixture(scope="module")
def rt():
    import torch
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return dict(torch=torch, lib=_lib)


def ref_of(kind, B, T, holes, scale=1024.0):
    """(cost, restatement's report), computed once per case and left unchanged"""
    key = (kind, B, T, holes, scale)
    if key not in REFS:
        cost = make_costs(kind, B, T, holes)
        cost.setflags(write=False)
        REFS[key] = (cost, assign_optimal_ref(cost, scale))
    return REFS[key]


def run(rt, cost, scale=1024.0, poison=-77, outputs=True, work=None, stream=None):
    """one call into poisoned outputs and a poisoned workspace: (assign, total, count, steps) as numpy / None"""
    torch, lib = rt["torch"], rt["lib"]
    cost = np.asarray(cost)
    G = 1 if cost.ndim == 2 else cost.shape[0]
    tc = _t(torch, cost)
    assign = torch.full(cost.shape[:-1], poison, dtype=torch.int32, device=DEV)
    total = torch.full((G,), poison, dtype=torch.int64, device=DEV) if outputs else None
    count = torch.full((G,), poison, dtype=torch.int32, device=DEV) if outputs else None
    steps = torch.full((G,), poison, dtype=torch.int32, device=DEV) if outputs else None
    if work is None:
        nbytes = lib.assign_optimal_work_bytes(G, cost.shape[-2], cost.shape[-1])
        work = torch.full((nbytes,), poison & 0xFF, dtype=torch.uint8, device=DEV)
    lib.assign_optimal_device(tc, assign, scale, total, count, steps, work, stream=stream)
    assert np.array_equal(tc.cpu().numpy(), cost, equal_nan=True)          # d_cost is untouched
    out = [t.cpu().numpy() if t is not None else None for t in (assign, total, count, steps)]
    return out


def same(got, want):
    a, total, count, steps = got
    assert np.array_equal(a, want[0]), np.flatnonzero(a != want[0])[:8]
    assert (int(total[0]), int(count[0]), int(steps[0])) == tuple(want[1:]), (total, count, steps, want[1:])


# a wave (64), a workgroup's wave count (65, 130, 257) and both orientations
SHAPES = [(1, 1), (1, 5), (5, 1), (3, 5), (5, 3), (64, 64), (65, 63), (63, 65), (130, 17), (17, 130), (257, 255)]


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_device_is_the_restatement(rt, kind, holes, B, T):
    cost, want = ref_of(kind, B, T, holes)
    same(run(rt, cost), want)
    if holes and min(B, T) > 1:
        assert want[2] < min(B, T) and (want[0] == -1).any()


# 2 and 4 columns per thread (4096 columns), 1024 threads with one column each, the limits of both sizes
@pytest.mark.parametrize("B,T", [(1024, 1024), (4096, 33), (33, 1024), (2000, 40)])
@pytest.mark.parametrize("kind", ["unif", "grid"])
def test_device_is_the_restatement_at_the_limits(rt, kind, B, T):
    cost, want = ref_of(kind, B, T, False)
    same(run(rt, cost), want)
    assert want[2] == min(B, T)


def test_all_untakeable_matrices(rt):
    for cost in (np.full((9, 4), INF), np.full((3, 3), NAN), -np.ones((4, 70)), np.full((130, 2), 1e9)):
        a, total, count, steps = run(rt, cost)
        assert (a == -1).all() and total[0] == 0 and count[0] == 0
        same((a, total, count, steps), assign_optimal_ref(cost))


def test_three_problems_in_one_call_are_the_three_lone_calls(rt):
    """G = 3 distinct problems, here with Qmax and P of their own; NULL optional outputs change nothing else; a second
    poison changes nothing"""
    for B, T in ((5, 3), (65, 63), (17, 130)):
        costs = np.stack([make_costs(k, B, T, h) for k, h in (("unif", True), ("ties", False), ("grid", True))])
        a, total, count, steps = run(rt, costs)
        for g in range(3):
            lone = run(rt, costs[g], poison=123456)
            assert np.array_equal(a[g], lone[0]) and (total[g], count[g], steps[g]) == (lone[1][0], lone[2][0], lone[3][0])
            same(lone, assign_optimal_ref(costs[g]))
        bare = run(rt, costs, poison=5, outputs=False)
        assert np.array_equal(bare[0], a) and bare[1] is None


def test_calls_on_a_side_stream_see_their_producer(rt):
    """the costs are written by a kernel on the side stream just ahead of each call, into a buffer that held other
    costs; the workspace is shared by the two calls"""
    torch, lib = rt["torch"], rt["lib"]
    B, T = 130, 70
    first, second = make_costs("unif", B, T, True), make_costs("grid", B, T, False)
    want = [assign_optimal_ref(first), assign_optimal_ref(second)]
    assert not np.array_equal(want[0][0], want[1][0])
    t1, t2 = _t(torch, first), _t(torch, second)
    work = torch.zeros(lib.assign_optimal_work_bytes(1, B, T), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(device=0)
    for _ in range(3):
        cost = torch.full((B, T), NAN, dtype=torch.float64, device=DEV)
        outs = []
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for src in (t1, t2):
                cost.copy_(src * 1.0)                                      # the producer
                assign = torch.full((B,), -5, dtype=torch.int32, device=DEV)
                total = torch.zeros(1, dtype=torch.int64, device=DEV)
                count, steps = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
                lib.assign_optimal_device(cost, assign, 1024.0, total, count, steps, work, stream=side.cuda_stream)
                outs.append((assign, total, count, steps))
        side.synchronize()
        for got, w in zip(outs, want):
            same([t.cpu().numpy() for t in got], w)


def test_scale_changes_q_as_the_restatement_says(rt):
    cost, want = ref_of("grid", 65, 63, False)
    coarse = assign_optimal_ref(cost, 1.0)
    same(run(rt, cost, 1.0), coarse)
    q1 = quantise(cost, 1.0)
    assert coarse[1] == q1[np.arange(65)[coarse[0] >= 0], coarse[0][coarse[0] >= 0]].sum()
    # either sum is within half a unit of q per pair of the true optimum
    assert want[1] != coarse[1] and abs(want[1] / 1024.0 - coarse[1]) <= 0.5 * 63 * (1.0 + 1.0 / 1024.0)


def test_goal_assigner_is_the_composed_restatement(rt):
    """shelf_map(), 16 robots and 24 goals on free cells, robot 3 on a walled-in cell: cost, assign and the routes equal
    field_ref -> route_costs_ref -> the restatement -> descend_ref; every route ends on its robot's goal; the goals are
    distinct; the optimal sum of quantised costs is at most greedy's and the fixed pairing's on the same matrix"""
    torch, lib = rt["torch"], rt["lib"]
    from robot_mpcs_amd.global_planner import GoalAssigner, RouteFollower, shelf_map
    data = shelf_map()
    H, W = data.shape
    B, T = 16, 24
    data[19:22, 29:32] = 1.0
    data[20, 30] = 0.0                                                     # free, shelf all around
    rng = np.random.default_rng(23)
    free = np.flatnonzero(data.ravel() < 0.8)
    free = free[free != 20 * W + 30]
    cells = rng.choice(free, B + T, replace=False).astype(np.int32)
    starts, goals = cells[:B].copy(), cells[B:]
    starts[3] = 20 * W + 30
    ga = GoalAssigner(_t(torch, data), goals)
    paths, lens = ga.plan(_t(torch, starts, torch.int32))
    assert paths is ga.paths and lens is ga.lens and ga.assignment.shape == (B,) and ga.cost.shape == (B, T)
    fields = np.stack([field_ref(data, int(g)) for g in goals])
    assert (ga.status == 0).all() and np.array_equal(ga.fields.cpu().numpy(), fields)
    cost = route_costs_ref(data, fields, starts)
    assert np.array_equal(ga.cost.cpu().numpy(), cost) and np.isinf(cost[3]).all()
    want = assign_optimal_ref(cost, ga.scale)
    a = ga.assignment.cpu().numpy()
    assert np.array_equal(a, want[0]) and (ga.total.item(), ga.count.item(), ga.steps.item()) == want[1:]
    assert a[3] == -1 and (np.delete(a, 3) >= 0).all() and len(set(np.delete(a, 3).tolist())) == B - 1
    P, L = paths.cpu().numpy(), lens.cpu().numpy()
    for b in range(B):
        if a[b] < 0:
            assert L[b] == 0
            continue
        route = descend_ref(data, fields[a[b]], int(starts[b]), int(goals[a[b]]))
        assert L[b] == len(route) and P[b, :L[b]].tolist() == route and route[-1] == goals[a[b]]
    gc = ga.goal_cells_of().cpu().numpy()
    assert np.array_equal(gc, np.where(a >= 0, goals[np.maximum(a, 0)], -1)) and gc.dtype == np.int32
    assert np.array_equal(ga.goal_cells_of(ga.assignment).cpu().numpy(), gc)
    # the same matrix under the two other pairings
    q = quantise(cost, ga.scale)
    greedy = greedy_ref(cost)[0]
    for other in (greedy, np.arange(B)):
        rows = np.flatnonzero((other >= 0) & (q[np.arange(B), np.maximum(other, 0)] >= 0))
        assert len(rows) == B - 1                                          # each pairs every robot but the walled-in one
        assert want[1] <= q[rows, other[rows]].sum()
    # the routes feed RouteFollower and RouteFollower.replace unchanged; assign alone gives the same pairing
    fol = RouteFollower(paths.clone(), lens.clone(), W, -9.0, -9.0, 0.45)
    fol.replace(paths, lens)
    assert torch.equal(fol.lens, lens) and torch.equal(ga.assign(_t(torch, starts, torch.int32)), _t(torch, a, torch.int32))


def test_example_runs_in_its_three_modes(rt):
    """examples/fleet_store_dispatch.py, 16 boxers and 24 pick cells, 30 control steps per mode: on the same cost matrix
    the optimal pairing's sum of q is at most greedy's and the fixed pairing's; measured on the MI355X over 400 steps
     the last arrival is at step 92 (fixed), 22 (greedy), 20 (optimal), so 30 steps see the optimal run
    arrive"""
    from example_loader import load_example
    ex = load_example("fleet_store_dispatch")
    out = {mode: ex.run(B=16, T=24, steps=30, seed=0, assign=mode) for mode in ex.MODES}
    for mode, r in out.items():
        print(r)
        assert r["fused"] and r["paired"] == r["routes"] == 16 and r["failed_solves"] == 0 and r["assign"] == mode, r
        assert set(r) - {"assign_steps"} == set(out["fixed"])
    q = {mode: r["route_cost_sum_q"] for mode, r in out.items()}
    assert q["optimal"] <= q["greedy"] and q["optimal"] <= q["fixed"], q
    assert out["optimal"]["arrivals"] == 16 and out["optimal"]["arrival_step_max"] <= 30 and out["optimal"]["assign_steps"] >= 16
    with pytest.raises(ValueError):
        ex.run(B=4, T=3, steps=1)
