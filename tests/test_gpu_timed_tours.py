"""Timed tours on the device (rmpc_timed_tours_plan_device, rmpc_timed_tours_follow_device, include/rmpc_timed_tours.h,
DESIGN.md 25) against the numpy restatement of tests/timed_tours_reference.py, bit for bit; every launch writes into
poisoned outputs and a workspace of 0xA5.  The restatement ranks end cells on the fields the device computed, so that
both compare the same doubles."""
import math

import numpy as np
import pytest

from example_loader import load_example
from gpu_support import DEV, _t
from timed_cases import random_tours_case as _random_case
from timed_reference import BAD_ORDER, OUTSIDE, conflicts
from timed_support import POISON, load_runtime, poisoned, same, stage, workspace
from timed_tours_reference import INT32_MAX, follow_ref, plan_ref, store_tours_case

pytestmark = pytest.mark.gpu

KEYS = ("paths", "status", "arrive", "serve_at", "served", "key", "unserved", "best")


@pytest.fixture(scope="module")
def rt():
    return load_runtime()


def _device_plan(rt, grid, starts, cells, stops, lens, park, orders, T, sep2, lag=1, dwell=0, movement=4, occ=0.8, stream=None,
                 work=None):
    """-> (device results as numpy, the restatement's) for the same fields"""
    torch, lib = rt["torch"], rt["lib"]
    stops = np.asarray(stops, dtype=np.int32).reshape(len(starts), -1)
    d = stage(rt, grid, cells, orders, movement, occ, stream, starts=starts, stops=stops, lens=lens, park=park)
    (G, B), (H, W) = d["orders"].shape, d["grid"].shape
    if work is None:
        work = workspace(torch, lib.timed_tours_work_bytes(H, W, T, G))
    out = poisoned(torch, KEYS, G, B, T, stops.shape[1])
    args = lib.timed_tours_args(d["grid"], d["starts"], d["stops"], d["lens"], d["park"], d["fields"], d["cells"], d["orders"],
                                work, out["paths"], out["status"], out["arrive"], out["key"], out["best"], out["serve_at"],
                                out["served"], out["unserved"], dwell=dwell, movement=movement, occ_threshold=occ, sep2=sep2,
                                lag=lag)
    lib.timed_tours_plan_device(args, stream=stream)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    want = plan_ref(np.asarray(grid, dtype=float), starts, stops, lens, park, d["fields"].cpu().numpy(),
                    np.asarray(cells, dtype=np.int32), orders, T, sep2, lag, dwell, movement, occ)
    return got, want


def _same(got, want, keys=KEYS):
    same(got, want, keys)


# ---- the plan ----------------------------------------------------------------------------------------------------------
def test_hand_cases(rt):
    z = np.zeros((1, 7))
    got, want = _device_plan(rt, z, [0], [3, 6], [[0, 1]], [2], [1], [[0]], 12, 1, dwell=2)
    _same(got, want)
    assert got["paths"][0, 0].tolist() == [0, 1, 2, 3, 3, 3, 4, 5, 6, 6, 6, 6, 6] and got["serve_at"][0, 0].tolist() == [3, 8]
    got, want = _device_plan(rt, z, [3], [3, 6], [[0, 1]], [2], [1], [[0]], 9, 1, dwell=2)          # the start on the stop
    _same(got, want)
    assert got["serve_at"][0, 0].tolist() == [0, 5]
    for dwell, at in ((0, [3, 3]), (1, [3, 4])):                                                    # one cell twice
        got, want = _device_plan(rt, z, [0], [3], [[0, 0]], [2], [0], [[0]], 8, 1, dwell=dwell)
        _same(got, want)
        assert got["serve_at"][0, 0].tolist() == at
    wall = z.copy()
    wall[0, 4] = 1.0
    got, want = _device_plan(rt, wall, [1], [2, 6, 0], [[0, 1, 2]], [3], [2], [[0]], 8, 1)          # a stop behind a wall
    _same(got, want)
    assert got["serve_at"][0, 0].tolist() == [1, -1, -1] and got["unserved"][0] == 2 and got["arrive"][0, 0] == 9
    got, want = _device_plan(rt, z, [3, 0], [3], [[0], [0]], [0, 1], [0, 0], [[0, 1], [1, 0]], 8, 1)    # a stop parked on
    _same(got, want)
    assert got["unserved"].tolist() == [1, 0] and got["best"][0] == 1
    got, want = _device_plan(rt, z, [0], [6], [[0]], [1], [0], [[0]], 7, 1, dwell=2)                # a + dwell > T
    _same(got, want)
    assert got["serve_at"][0, 0].tolist() == [-1] and got["paths"][0, 0].tolist() == [0, 1, 2, 3, 4, 5, 6, 6]
    got, want = _device_plan(rt, np.zeros((5, 5)), [2, 12], [22, 12], [[0], [1]], [0, 1], [0, 1], [[0, 1]], 10, 1, dwell=2)
    _same(got, want)                                                                                # held fails, then passes
    assert got["serve_at"][0, 1].tolist() == [4]
    g = np.ones((3, 7))
    g[1, :] = 0.0
    g[0, 5] = 0.0
    got, want = _device_plan(rt, g, [7, 13], [13, 7, 5], [[0], [2]], [0, 1], [0, 1], [[0, 1]], 14, 1, dwell=1)
    _same(got, want)                                                                                # the swap corridor
    assert got["paths"][0, 1].tolist() == [13, 12, 5, 5, 5, 5, 5, 12, 11, 10, 9, 8, 7, 7, 7]
    got, want = _device_plan(rt, np.zeros((1, 3)), [2, 0], [0, 2], [[0], [1]], [0, 1], [0, 1], [[0, 1]], 5, 1)
    _same(got, want)                                                                                # a leg on an empty layer
    assert got["status"][0].tolist() == [0, 1] and got["paths"][0, 1].tolist() == [0] * 6 and got["unserved"][0] == 1


@pytest.mark.parametrize("name,H,W,B,T,G,K,movement,lag,sep2,dwell", [
    ("small", 7, 5, 3, 9, 2, 2, 4, 1, 2, 1),
    ("eight-moves-lag-2-dwell-0", 12, 9, 5, 20, 2, 3, 8, 2, 4, 0),
    ("eight-moves-lag-2-dwell-1", 12, 9, 5, 20, 2, 3, 8, 2, 4, 1),
    ("eight-moves-lag-2-dwell-3", 12, 9, 5, 20, 2, 3, 8, 2, 4, 3),
    ("word-and-lane-seams", 65, 70, 6, 40, 2, 2, 8, 1, 5, 2),          # two words per row; the history in LDS
    ("history-in-the-workspace", 65, 70, 6, 70, 2, 2, 4, 1, 5, 2),     # 71 layers of 130 words: beyond the history's LDS
    ("three-words-per-row", 4, 130, 4, 40, 2, 2, 8, 1, 4, 1),
    ("128-threads", 100, 20, 4, 30, 2, 2, 4, 3, 10, 1),                # 100 words per layer
    ("one-layer", 7, 5, 3, 1, 2, 2, 4, 1, 2, 0),
    ("dwell-64", 65, 70, 4, 70, 2, 2, 8, 1, 5, 64),                    # one stop fits the window, a second one cannot
])
def test_plan_is_the_restatement(rt, name, H, W, B, T, G, K, movement, lag, sep2, dwell):
    c, rng = _random_case(H, W, B, K, 7 * H + W + T, sep2=sep2)
    orders = [np.arange(B)] + [rng.permutation(B) for _ in range(G - 1)]
    got, want = _device_plan(rt, orders=orders, T=T, sep2=sep2, lag=lag, dwell=dwell, movement=movement, **c)
    _same(got, want)
    assert np.all(got["status"] >= 0)
    if name != "one-layer":
        assert got["served"].sum() > 0


def test_sixty_four_stops_of_which_one_is_used(rt):
    c, rng = _random_case(7, 5, 3, 64, 11, sep2=2, lens=1)
    got, want = _device_plan(rt, orders=[[0, 1, 2], [2, 0, 1]], T=9, sep2=2, dwell=1, **c)
    _same(got, want)
    assert got["serve_at"].shape == (2, 3, 64) and (got["serve_at"][:, :, 1:] == -1).all() and got["served"].sum() > 0


def test_nan_cells_are_free_and_the_threshold_is_inclusive(rt):
    c, rng = _random_case(9, 9, 3, 2, 5)
    c["grid"][c["grid"] > 0.5] = 0.8
    c["grid"][4, 4] = math.nan
    c["cells"][0] = 4 * 9 + 4                         # the NaN cell is a stop
    got, want = _device_plan(rt, orders=[[2, 0, 1]], T=20, sep2=4, dwell=1, **c)
    _same(got, want)


def test_a_skipped_robot_of_each_kind(rt):
    g = np.zeros((4, 4))
    starts = [0, -1, 3, 12, 15, 16]
    stops = [[0, 1], [0, 1], [0, 2], [0, 1], [1, -1], [0, 1]]
    got, want = _device_plan(rt, g, starts, [5, 10], stops, [2, 1, 2, 3, 2, -1], [1, 1, 1, 1, 0, 2],
                             [np.arange(6), np.arange(6)[::-1]], 9, 1)
    _same(got, want)
    assert got["status"][0].tolist() == [0] + [OUTSIDE] * 5 and got["unserved"][0] == 5
    assert (got["paths"][:, 1:] == -1).all() and (got["serve_at"][:, 1:] == -1).all()


def test_rows_that_are_no_permutations(rt):
    c, rng = _random_case(7, 5, 3, 2, 3, sep2=2)
    got, want = _device_plan(rt, orders=[[0, 1, 2], [0, 3, 1], [2, 1, 0]], T=9, sep2=2, dwell=1, **c)
    _same(got, want)
    assert got["status"][1].tolist() == [BAD_ORDER] * 3 and got["unserved"][1] == INT32_MAX and got["best"][0] in (0, 2)
    assert (got["serve_at"][1] == -1).all() and (got["served"][1] == 0).all()
    got, want = _device_plan(rt, orders=[[1, 1, 0], [-1, 0, 1]], T=9, sep2=2, dwell=1, **c)
    _same(got, want)
    assert got["best"][0] == -1


def test_twice_on_one_workspace_and_on_a_side_stream(rt):
    torch, lib = rt["torch"], rt["lib"]
    c, rng = _random_case(12, 9, 5, 3, 21)
    orders = [np.arange(5), rng.permutation(5)]
    work = workspace(torch, lib.timed_tours_work_bytes(12, 9, 20, 2))
    a, want = _device_plan(rt, orders=orders, T=20, sep2=4, dwell=1, movement=8, work=work, **c)
    _same(a, want)
    b, _ = _device_plan(rt, orders=orders, T=20, sep2=4, dwell=1, movement=8, work=work, **c)     # what the first left in it
    _same(b, a)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # (the copies of the inputs run on it too)
        s, _ = _device_plan(rt, orders=orders, T=20, sep2=4, dwell=1, movement=8, stream=side.cuda_stream, **c)
    _same(s, a)


@pytest.mark.parametrize("H,W,B,T,movement,lag,sep2", [(7, 5, 3, 9, 4, 1, 2), (12, 9, 5, 20, 8, 2, 4)])
def test_without_stops_it_is_the_timed_plan_itself(rt, H, W, B, T, movement, lag, sep2):
    torch, lib = rt["torch"], rt["lib"]
    c, rng = _random_case(H, W, B, 2, 7 * H + W + T, sep2=sep2, lens=0)
    orders = np.stack([np.arange(B), rng.permutation(B)]).astype(np.int32)
    got, want = _device_plan(rt, orders=orders, T=T, sep2=sep2, lag=lag, dwell=2, movement=movement, **c)
    _same(got, want)
    i32 = torch.int32
    d_grid, d_cells = _t(torch, c["grid"]), _t(torch, c["cells"], i32)
    fields = torch.empty((len(c["cells"]), H, W), dtype=torch.float64, device=DEV)
    lib.grid_fields_device(d_grid, d_cells, fields, torch.empty(len(c["cells"]), dtype=i32, device=DEV), movement, 0.8, 3.0)
    out = poisoned(torch, ("paths", "status", "arrive", "key", "best"), 2, B, T)
    work = workspace(torch, lib.timed_plan_work_bytes(H, W, T, 2))
    args = lib.timed_plan_args(d_grid, _t(torch, c["starts"], i32), _t(torch, c["park"], i32), fields, d_cells,
                               _t(torch, orders, i32), work, out["paths"], out["status"], out["arrive"], out["key"], out["best"],
                               movement=movement, sep2=sep2, lag=lag)
    lib.timed_plan_device(args)
    torch.cuda.synchronize()
    for k in ("paths", "status", "arrive", "key", "best"):
        assert np.array_equal(got[k], out[k].cpu().numpy()), k
    assert (got["unserved"] == 0).all() and (got["serve_at"] == -1).all() and (got["arrive"] <= T).any()


# ---- the store case through the Python layer -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store(rt):
    """the store case of tests/test_timed_tours_cpu.py through ``TourPlanner`` and ``TimedTours``, and the composed
    restatements: the tours of tests/tours_reference.py, then ``plan_ref`` on the device's fields"""
    import tours_reference
    torch = rt["torch"]
    from robot_mpcs_amd.global_planner import TimedTours, TourPlanner, priority_orders
    raw, g_inf, starts, picks = store_tours_case(16, 24, 0, 9)
    tp = TourPlanner(g_inf, picks, 2, device=DEV)
    tt = TimedTours(tp, 255, 9, lag=1, dwell=3, orders=16, park="last", seed=0)
    paths, serve_at, status, served, arrive, best = tt.plan(starts)
    torch.cuda.synchronize()
    got = dict(paths=paths, serve_at=serve_at, status=status, served=served, arrive=arrive, best=best, key=tt.key,
               unserved=tt.unserved)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    ref = tours_reference.plan_ref(g_inf, starts, picks, 2)
    tours, lens = ref["out"]["tours"], ref["out"]["len"]
    park = np.where(lens > 0, tours[np.arange(16), np.maximum(lens, 1) - 1], 24 + np.arange(16)).astype(np.int32)
    cells = np.concatenate([picks, starts]).astype(np.int32)
    want = plan_ref(g_inf, starts, tours, lens, park, tt.fields.cpu().numpy(), cells, priority_orders(16, 16, 0), 255, 9, 1, 3, 8)
    return dict(tt=tt, tp=tp, got=got, want=want, tours=tours, lens=lens, park=park, cells=cells, starts=starts, picks=picks)


def test_timed_tours_plan_is_the_composed_restatements(rt, store):
    tt, tp = store["tt"], store["tp"]
    assert np.array_equal(tp.tours.cpu().numpy(), store["tours"]) and np.array_equal(tp.tour_len.cpu().numpy(), store["lens"])
    assert np.array_equal(tt.park_index.cpu().numpy(), store["park"]) and np.array_equal(tt.goal_cells.cpu().numpy(), store["cells"])
    _same(store["got"], store["want"])
    # a second plan with the same object reuses the workspace whatever the first left in it
    again = tt.plan(store["starts"])
    rt["torch"].cuda.synchronize()
    assert np.array_equal(again[0].cpu().numpy(), store["got"]["paths"])


def test_guarantee_on_the_best_order_of_the_store_case(store):
    from robot_mpcs_amd.store import STORE
    got = store["got"]
    b = int(got["best"][0])
    assert got["unserved"][b] == 0 and got["status"][b].tolist() == [0] * 16 and got["served"][b].sum() == 24
    assert conflicts(got["paths"][b], got["status"][b], STORE.W, 9, 1) == []
    sa = got["serve_at"][b]
    for r in range(16):
        n = int(store["lens"][r])
        assert (sa[r, :n] >= 0).all() and (np.diff(sa[r, :n]) >= 3).all()
        for j in range(n):
            assert (got["paths"][b, r, sa[r, j]:sa[r, j] + 4] == store["picks"][store["tours"][r, j]]).all()


# ---- the follower ------------------------------------------------------------------------------------------------------
def _device_follow(rt, paths, idx_in, pos, goal, W, x0, y0, cell, threshold, sep2, lag, serve_at, leg, served, now, stop_tol,
                   with_blocked=True):
    torch, lib = rt["torch"], rt["lib"]
    i32 = torch.int32
    B = len(paths)
    d_out = torch.full((B,), POISON, dtype=i32, device=DEV)
    d_goal, d_leg, d_served = _t(torch, goal), _t(torch, np.asarray(leg), i32), _t(torch, np.asarray(served), i32)
    d_blk = torch.full((B,), POISON, dtype=i32, device=DEV) if with_blocked else None
    lib.timed_tours_follow_device(_t(torch, paths, i32), _t(torch, np.asarray(idx_in), i32), d_out, _t(torch, pos), d_goal, W, x0,
                                  y0, cell, threshold, sep2, lag, _t(torch, np.asarray(serve_at), i32), d_leg, d_served, now,
                                  stop_tol, blocked=d_blk)
    torch.cuda.synchronize()
    return (d_out.cpu().numpy(), d_goal.cpu().numpy(), None if d_blk is None else d_blk.cpu().numpy(), d_leg.cpu().numpy(),
            d_served.cpu().numpy())


def test_follower_on_constructed_indices(rt):
    paths = np.array([[0, 1, 2, 2], [2, 2, 2, 2], [-1, -1, -1, -1], [2, 2, 2, 2], [5, 6, 6, 7]], np.int32)
    pos = np.array([[1.0, 0.0, 9.0], [2.0, 0.0, 9.0], [9.0, 9.0, 9.0], [2.05, 0.0, 9.0], [1.0, 1.0, 9.0]])     # (stride 3)
    sa = np.array([[2, -1], [0, 0], [0, 1], [1, 3], [1, 2]], np.int32)
    goal = np.full((5, 3), 7.0)
    served = np.full((5, 2), -1, np.int32)
    cases = [([1, 0, 5, 0, 1], [0, 0, 0, 0, 0]), ([2, 0, 5, 1, 1], [0, 1, 0, 0, 0]), ([2, 1, 5, 1, 2], [1, 2, 0, 1, 1]),
             ([-4, 9, 0, 3, 9], [0, 0, 1, 1, -2]), ([0, 0, 0, 0, 0], [2, 2, 2, 2, 2]), ([2, 0, 0, 3, 1], [0, 0, 0, 1, 0])]
    for idx_in, leg in cases:
        for tol in (0.02, 0.1):
            want = follow_ref(paths, idx_in, pos, goal, 5, 0.0, 0.0, 1.0, 0.3, 1, 1, sa, leg, served, 6, tol)
            got = _device_follow(rt, paths, idx_in, pos, goal, 5, 0.0, 0.0, 1.0, 0.3, 1, 1, sa, leg, served, 6, tol)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (idx_in, leg, tol, got, want)
    want = follow_ref(paths, [1, 0, 5, 1, 1], pos, goal, 5, 0.0, 0.0, 1.0, 0.3, 1, 1, sa, [0] * 5, served, 2, 0.1)
    got = _device_follow(rt, paths, [1, 0, 5, 1, 1], pos, goal, 5, 0.0, 0.0, 1.0, 0.3, 1, 1, sa, [0] * 5, served, 2, 0.1,
                         with_blocked=False)
    assert got[2] is None and all(np.array_equal(got[i], want[i]) for i in (0, 1, 3, 4))
    assert (want[4] >= 0).any()


def test_follower_through_a_scripted_sequence(rt, store):
    """40 steps at B = 16 on the store's best order through ``TimedTourFollower``: the positions of every step are given
    (each robot moves a fixed share of the way to its goal; the first robot whose route leaves its start at layer 1
    stands still for the first 15 steps); the indices, goals, blocked, legs and served of every step are the
    restatement's."""
    torch = rt["torch"]
    from robot_mpcs_amd.global_planner import TimedTourFollower
    from robot_mpcs_amd.store import STORE as S
    b = int(store["got"]["best"][0])
    paths, sa, starts = store["got"]["paths"][b], store["got"]["serve_at"][b], store["starts"]
    fol = TimedTourFollower(_t(torch, paths, torch.int32), _t(torch, sa, torch.int32), S.W, S.x0, S.y0, S.cell, 0.3, 0.1, 9, 1)
    pos = np.stack([S.x0 + (starts % S.W) * S.cell, S.y0 + (starts // S.W) * S.cell, np.zeros(16)], 1)
    goal = np.full((16, 3), math.nan)
    idx, leg, served = np.zeros(16, np.int32), np.zeros(16, np.int32), np.full((16, 2), -1, np.int32)
    d_goal = _t(torch, goal)
    held = int(np.flatnonzero(paths[:, 1] != paths[:, 0])[0])
    for step in range(40):
        idx, goal, blk, leg, served = follow_ref(paths, idx, pos, goal, S.W, S.x0, S.y0, S.cell, 0.3, 9, 1, sa, leg, served,
                                                 step, 0.1)
        fol.step(_t(torch, pos), d_goal)
        torch.cuda.synchronize()
        assert np.array_equal(fol.idx.cpu().numpy(), idx), step
        assert np.array_equal(d_goal.cpu().numpy(), goal), step
        assert np.array_equal(fol.blocked.cpu().numpy(), blk), step
        assert np.array_equal(fol.leg.cpu().numpy(), leg) and np.array_equal(fol.served.cpu().numpy(), served), step
        move = np.full((16, 1), 0.8)
        if step < 15:
            move[held] = 0.0
        pos[:, :2] += move * (goal[:, :2] - pos[:, :2])
    assert idx.max() > 10 and idx[held] <= 26 and (served >= 0).sum() > 0      # (one layer per step once it moves)
    assert int(fol.served_count().item()) == (served >= 0).sum()


def test_follower_without_stops_is_the_timed_follower(rt, store):
    torch, lib = rt["torch"], rt["lib"]
    from robot_mpcs_amd.store import STORE as S
    i32 = torch.int32
    rng = np.random.default_rng(1)
    paths = store["got"]["paths"][0]
    for trial in range(3):
        idx = rng.integers(-1, 60, 16).astype(np.int32)
        c = paths[np.arange(16), np.clip(idx, 0, 255)]
        pos = np.stack([S.x0 + (c % S.W) * S.cell + rng.choice([0.0, 0.2], 16), S.y0 + (c // S.W) * S.cell], 1)
        goal = rng.uniform(size=(16, 3))
        leg, served = rng.integers(0, 3, 16), rng.integers(-1, 5, (16, 2))
        got = _device_follow(rt, paths, idx, pos, goal, S.W, S.x0, S.y0, S.cell, 0.3, 9, 1, np.full((16, 2), -1), leg, served,
                             3, 0.05)
        d_out, d_goal = torch.full((16,), POISON, dtype=i32, device=DEV), _t(torch, goal)
        d_blk = torch.full((16,), POISON, dtype=i32, device=DEV)
        lib.timed_follow_device(_t(torch, paths, i32), _t(torch, idx, i32), d_out, _t(torch, pos), d_goal, S.W, S.x0, S.y0,
                                S.cell, 0.3, 9, 1, blocked=d_blk)
        torch.cuda.synchronize()
        assert np.array_equal(got[0], d_out.cpu().numpy()) and np.array_equal(got[1], d_goal.cpu().numpy())
        assert np.array_equal(got[2], d_blk.cpu().numpy())
        assert np.array_equal(got[3], leg) and np.array_equal(got[4], served)
        assert (got[0] != np.clip(idx, 0, 255)).any()


# ---- closed loop -------------------------------------------------------------------------------------------------------
def test_closed_loop_timed_tours(rt):
    """16 boxers serve 24 picks in the store (examples/fleet_store_timed_tours.py, seed 0, K = 2, dwell 3, 16 orders) on
    timed tours, with the separating planes beside the lidar planes, over at most 400 control steps, the budget of the
    closed loop of tests/test_gpu_tours.py.  Gates: every planned pick is served and all 24 are planned, at most 1 % of
    the robot-steps failed, no base centre inside a shelf, no pair of end links closer than r_i + r_j - 1e-3 m, and
    every robot stood at least ``dwell`` consecutive steps on each of its picks.  The step of the last service and the
    figures of the static plan are in DESIGN.md 25, not asserted."""
    ex = load_example("fleet_store_timed_tours")
    out = ex.run(B=16, picks=24, K=2, steps=400, seed=0, plan="timed", dwell=3)
    print(out)
    assert out["plan_failures"] == 0 and out["plan_unserved"] == 0, out
    assert out["picks_planned"] == 24 and out["picks_served"] == 24, out
    assert out["failed_share"] <= 0.01, out
    assert out["base_inside"] == 0 and out["min_base_clearance_m"] > 0.0, out
    assert out["min_pair_gap_m"] >= -1e-3, out
    assert out["min_steps_on_a_pick"] >= 3, out
