"""The timed routes on the device (rmpc_timed_plan_device, rmpc_timed_follow_device) against the numpy
restatement of tests/timed_reference.py, bit for bit; every launch writes into poisoned outputs.  The restatement ranks
end cells on the fields the device computed, so that both compare the same doubles."""
import math

import numpy as np
import pytest

from example_loader import load_example
from gpu_support import DEV, _t
from timed_cases import random_case as _random_case
from timed_reference import BAD_ORDER, OUTSIDE, conflicts, fields_for, follow_ref, plan_ref, store_case
from timed_support import POISON, goal_index, load_runtime, poisoned, same, stage, workspace

pytestmark = pytest.mark.gpu

KEYS = ("paths", "status", "arrive", "key", "best")


@pytest.fixture(scope="module")
def rt():
    return load_runtime()


def _device_plan(rt, grid, starts, goals, orders, T, sep2, lag=1, movement=4, occ=0.8, stream=None):
    """-> (device results as numpy, the restatement's) for the same fields"""
    torch, lib = rt["torch"], rt["lib"]
    goal_cells, gi = goal_index(goals)
    d = stage(rt, grid, goal_cells, orders, movement, occ, stream, starts=starts, gi=gi)
    (G, B), (H, W) = d["orders"].shape, d["grid"].shape
    work = workspace(torch, lib.timed_plan_work_bytes(H, W, T, G))
    out = poisoned(torch, KEYS, G, B, T)
    args = lib.timed_plan_args(d["grid"], d["starts"], d["gi"], d["fields"], d["cells"], d["orders"], work, out["paths"],
                               out["status"], out["arrive"], out["key"], out["best"], movement=movement, occ_threshold=occ,
                               sep2=sep2, lag=lag)
    lib.timed_plan_device(args, stream=stream)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    want = plan_ref(np.asarray(grid, dtype=float), starts, gi, d["fields"].cpu().numpy(), goal_cells, orders, T, sep2, lag,
                    movement, occ)
    return got, want


def _same(got, want):
    same(got, want, KEYS)


# ---- the plan ----------------------------------------------------------------------------------------------------------
def test_hand_cases(rt):
    got, want = _device_plan(rt, np.zeros((1, 7)), [0, 6], [6, 0], [[0, 1]], 8, 1)
    _same(got, want)
    assert got["status"][0].tolist() == [0, 5] and got["paths"][0, 1].tolist() == [6] * 9
    g = np.ones((3, 7))
    g[1, :] = 0.0
    g[0, 5] = 0.0
    got, want = _device_plan(rt, g, [7, 13], [13, 7], [[0, 1]], 14, 1)
    _same(got, want)
    assert got["paths"][0, 1].tolist() == [13, 12, 5, 5, 5, 5, 5, 12, 11, 10, 9, 8, 7, 7, 7]


@pytest.mark.parametrize("name,H,W,B,T,G,movement,lag,sep2", [
    ("small", 7, 5, 3, 9, 2, 4, 1, 2),
    ("eight-moves-lag-2", 12, 9, 5, 20, 2, 8, 2, 4),
    ("word-and-lane-seams", 65, 70, 6, 40, 2, 8, 1, 5),          # two words per row, more rows than a wave has lanes
    ("history-in-the-workspace", 65, 70, 6, 70, 2, 4, 1, 5),     # 71 layers of 130 words: beyond the history's LDS
    ("three-words-per-row", 4, 130, 4, 40, 2, 8, 1, 4),
    ("128-threads", 100, 20, 4, 30, 2, 4, 3, 10),                # 100 words per layer
    ("one-layer", 7, 5, 3, 1, 2, 4, 1, 2),
    ("one-robot", 7, 5, 1, 9, 1, 8, 4, 2),
])
def test_plan_is_the_restatement(rt, name, H, W, B, T, G, movement, lag, sep2):
    g, starts, goals, rng = _random_case(H, W, B, 7 * H + W + T, sep2=sep2)
    orders = [np.arange(B)] + [rng.permutation(B) for _ in range(G - 1)]
    got, want = _device_plan(rt, g, starts, goals, orders, T, sep2, lag, movement)
    _same(got, want)
    assert np.all(got["status"] >= 0)


def test_nan_cells_are_free_and_the_threshold_is_inclusive(rt):
    g, starts, goals, rng = _random_case(9, 9, 3, 5)
    g[g > 0.5] = 0.8
    g[4, 4] = math.nan
    got, want = _device_plan(rt, g, starts, goals, [[2, 0, 1]], 20, 4)
    _same(got, want)


def test_store_plan_through_timed_routes(rt):
    """the store case of tests/test_timed_cpu.py, G = 4, through the Python layer; the guarantee on the device's best"""
    torch = rt["torch"]
    from robot_mpcs_amd.global_planner import TimedRoutes, priority_orders
    from robot_mpcs_amd.store import STORE
    raw, g_inf, starts, goals = store_case(16, 0, 9)
    tr = TimedRoutes(g_inf, 4, 0.8, 128, 9, lag=1, orders=4, device=DEV)
    paths, status, arrive, best = tr.plan(starts, goals)
    torch.cuda.synchronize()
    orders = priority_orders(16, 4, 0)
    assert np.array_equal(tr.orders.cpu().numpy(), orders) and np.array_equal(orders[0], np.arange(16))
    goal_cells, gi = np.unique(goals), np.searchsorted(np.unique(goals), goals)
    want = plan_ref(g_inf, starts, gi, tr.fields.cpu().numpy(), goal_cells, orders, 128, 9, 1, 4)
    got = dict(paths=paths.cpu().numpy(), status=status.cpu().numpy(), arrive=arrive.cpu().numpy(),
               key=tr.key.cpu().numpy(), best=best.cpu().numpy())
    _same(got, want)
    b = int(got["best"][0])
    assert got["status"][0].tolist() == [0] * 16 and got["status"][b].tolist() == [0] * 16
    assert conflicts(got["paths"][b], got["status"][b], STORE.W, 9, 1) == []
    # a second plan with the same object reuses the workspace whatever the first left in it
    again = tr.plan(starts, goals)
    torch.cuda.synchronize()
    assert np.array_equal(again[0].cpu().numpy(), got["paths"])


def test_a_row_that_is_no_permutation(rt):
    g, starts, goals, rng = _random_case(7, 5, 3, 3, sep2=2)
    got, want = _device_plan(rt, g, starts, goals, [[0, 1, 2], [0, 3, 1], [2, 1, 0]], 9, 2)
    _same(got, want)
    assert got["status"][1].tolist() == [BAD_ORDER] * 3 and got["best"][0] in (0, 2)
    got, want = _device_plan(rt, g, starts, goals, [[1, 1, 0], [-1, 0, 1]], 9, 2)
    _same(got, want)
    assert got["best"][0] == -1


def test_a_skipped_robot_and_an_unreachable_goal(rt):
    g = np.zeros((7, 7))
    g[:, 4] = 1.0                                      # a wall: columns 5, 6 cannot be reached from the left
    starts, goals = [0, -1, 14, 49], [21, 3, 6, 2]     # robot 1 starts outside, robot 2's goal lies behind the wall,
    got, want = _device_plan(rt, g, starts, goals, [[0, 1, 2, 3], [3, 2, 1, 0]], 12, 2)   # robot 3 starts past the map
    _same(got, want)
    assert got["status"][0].tolist() == [0, OUTSIDE, 0, OUTSIDE]
    assert got["arrive"][0, 2] == 13 and np.all(got["paths"][0, 1] == -1)


def test_side_stream_equals_default_stream(rt):
    torch = rt["torch"]
    g, starts, goals, rng = _random_case(12, 9, 5, 21)
    orders = [np.arange(5), rng.permutation(5)]
    a, want = _device_plan(rt, g, starts, goals, orders, 20, 4, 1, 8)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # (the copies of the inputs run on it too)
        b, _ = _device_plan(rt, g, starts, goals, orders, 20, 4, 1, 8, stream=side.cuda_stream)
    _same(a, want)
    _same(b, a)


def test_refusals(rt):
    torch, lib = rt["torch"], rt["lib"]
    i32 = torch.int32
    z = lambda *s, dt=i32: torch.zeros(s, dtype=dt, device=DEV)
    grid, fields = z(4, 4, dt=torch.float64), z(1, 4, 4, dt=torch.float64)
    work = z(lib.timed_plan_work_bytes(4, 4, 5, 1), dt=torch.uint8)

    def args(T=5, sep2=1, lag=1, movement=4, work=work):
        return lib.timed_plan_args(grid, z(2), z(2), fields, z(1), z(1, 2), work, z(1, 2, T + 1), z(1, 2), z(1, 2),
                                   z(1, dt=torch.int64), z(1), movement=movement, sep2=sep2, lag=lag)
    for bad in (dict(sep2=0), dict(sep2=lib.TIMED_MAX_SEP2 + 1), dict(lag=0), dict(lag=5), dict(movement=6),
                dict(T=lib.TIMED_MAX_T + 1), dict(work=work[:-8])):
        with pytest.raises(lib.RmpcError):
            lib.timed_plan_device(args(**bad))
    a = args()
    a.struct_size -= 1
    with pytest.raises(lib.RmpcError):
        lib.timed_plan_device(a)
    with pytest.raises(lib.RmpcError):
        lib.timed_plan_work_bytes(129, 128, 5, 1)
    idx = z(2)
    with pytest.raises(lib.RmpcError):                 # one buffer for both indices
        lib.timed_follow_device(z(2, 6), idx, idx, z(2, 2, dt=torch.float64), z(2, 3, dt=torch.float64), 4, 0.0, 0.0, 1.0,
                                0.5, 1, 1)
    lib.timed_plan_device(args())                      # (the arguments the refusals vary are fine)
    torch.cuda.synchronize()


# ---- the follower ------------------------------------------------------------------------------------------------------
def _device_follow(rt, paths, idx_in, pos, goal, W, x0, y0, cell, threshold, sep2, lag, with_blocked=True):
    torch, lib = rt["torch"], rt["lib"]
    B = len(paths)
    d_out = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    d_goal = _t(torch, goal)
    d_blk = torch.full((B,), POISON, dtype=torch.int32, device=DEV) if with_blocked else None
    lib.timed_follow_device(_t(torch, paths, torch.int32), _t(torch, idx_in, torch.int32), d_out, _t(torch, pos), d_goal, W,
                            x0, y0, cell, threshold, sep2, lag, blocked=d_blk)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_goal.cpu().numpy(), None if d_blk is None else d_blk.cpu().numpy()


def test_follower_on_constructed_indices(rt):
    paths = np.array([[0, 1, 2, 2], [2, 2, 2, 2], [-1, -1, -1, -1], [2, 2, 2, 2]], np.int32)
    pos = np.array([[1.0, 0.0, 9.0], [2.0, 0.0, 9.0], [9.0, 9.0, 9.0], [2.0, 0.0, 9.0]])        # (stride 3)
    goal = np.full((4, 3), 7.0)
    for idx_in in ([1, 0, 5, 0], [1, 1, 5, 0], [1, 1, 5, 1], [-4, 9, 0, 3], [0, 0, 0, 0]):
        want = follow_ref(paths, idx_in, pos, goal, 5, 0.0, 0.0, 1.0, 0.1, 1, 1)
        got = _device_follow(rt, paths, idx_in, pos, goal, 5, 0.0, 0.0, 1.0, 0.1, 1, 1)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (idx_in, got, want)
    B3 = paths[[0, 1, 3]]
    want = follow_ref(B3, [1, 0, 0], pos[:3], goal[:3], 5, 0.0, 0.0, 1.0, 0.1, 1, 1)
    got = _device_follow(rt, B3, [1, 0, 0], pos[:3], goal[:3], 5, 0.0, 0.0, 1.0, 0.1, 1, 1, with_blocked=False)
    assert got[2] is None and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert want[2].tolist() == [1, -1, -1]


def test_follower_through_a_scripted_sequence(rt):
    """40 steps at B = 16 on the store plan through ``TimedFollower``: the positions of every step are given (each robot
    moves a fixed share of the way to its goal; robot 3 stands still for the first 15 steps), the indices, goals and
    blocked of every step are the restatement's."""
    torch = rt["torch"]
    from robot_mpcs_amd.global_planner import TimedFollower
    from robot_mpcs_amd.store import STORE as S
    raw, g_inf, starts, goals = store_case(16, 0, 9)
    goal_cells, gi = np.unique(goals), np.searchsorted(np.unique(goals), goals)
    plan = plan_ref(g_inf, starts, gi, fields_for(g_inf, goal_cells, 4), goal_cells, [np.arange(16)], 128, 9, 1, 4)
    paths = plan["paths"][0]
    fol = TimedFollower(_t(torch, paths, torch.int32), S.W, S.x0, S.y0, S.cell, 0.3, 9, 1)
    pos = np.stack([S.x0 + (starts % S.W) * S.cell, S.y0 + (starts // S.W) * S.cell, np.zeros(16)], 1)
    goal = np.full((16, 3), math.nan)
    idx = np.zeros(16, np.int32)
    d_goal = _t(torch, goal)
    blocked_seen = 0
    for step in range(40):
        idx, goal, blk = follow_ref(paths, idx, pos, goal, S.W, S.x0, S.y0, S.cell, 0.3, 9, 1)
        fol.step(_t(torch, pos), d_goal)
        torch.cuda.synchronize()
        assert np.array_equal(fol.idx.cpu().numpy(), idx), step
        assert np.array_equal(d_goal.cpu().numpy(), goal), step
        assert np.array_equal(fol.blocked.cpu().numpy(), blk), step
        blocked_seen += int((blk >= 0).sum())
        move = np.full((16, 1), 0.8)
        if step < 15:
            move[3] = 0.0
        pos[:, :2] += move * (goal[:, :2] - pos[:, :2])
    assert idx.max() > 10 and idx[3] <= 25


# ---- closed loop -------------------------------------------------------------------------------------------------------
def test_closed_loop_timed_routes_against_plain_routes(rt):
    """16 boxers cross the store (examples/fleet_store_timed.py, seed 0) with separating planes beside the lidar planes,
    once on the plain routes of ``RouteFollower`` and once on timed routes, from the same starts to the same goals.  The
    plain run gives the last arrival A; both runs are then compared over ceil(1.35 A) steps.  Safety gates of the store
    and fleet-planes tests on the timed run: at most 1 % of the robot-steps failed, no base centre inside a shelf, no
    pair of robots closer than r_i + r_j - 1e-3.  The timed run brings home at least as many robots as the plain one,
    more when the plain one leaves anyone out.  Measured on an MI355X: A = 86, 117 steps; plain 6 of 16
    arrive, 6.4 % failed robot-steps, pairs overlap by 0.27 m; timed 15 of 16 (16 by step 119), no failed solve, the least
    pair distance r_i + r_j + 1.7e-7 m."""
    ex = load_example("fleet_store_timed")
    first = ex.run(B=16, steps=260, seed=0, mode="plain")
    print(first)
    assert first["arrivals"] >= 1, first
    steps = math.ceil(1.35 * first["arrival_step_max"])
    plain = ex.run(B=16, steps=steps, seed=0, mode="plain")
    timed = ex.run(B=16, steps=steps, seed=0, mode="timed")
    print(plain)
    print(timed)
    assert timed["plan_failures"] == 0, timed
    assert timed["failed_share"] <= 0.01, timed
    assert timed["base_inside"] == 0 and timed["min_base_clearance_m"] > 0.0, timed
    assert timed["min_pair_gap_m"] >= -1e-3, timed
    assert timed["arrivals"] >= plain["arrivals"], (timed, plain)
    if plain["arrivals"] < 16:
        assert timed["arrivals"] > plain["arrivals"], (timed, plain)
