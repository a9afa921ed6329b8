"""The repair of failing priority orders on the device (rmpc_timed_plan_repair_device) against the numpy
restatement of tests/timed_repair_reference.py, bit for bit; every launch writes into poisoned outputs and a workspace
filled with 0xA5.  The restatement ranks end cells on the fields the device computed, so that both compare the same
doubles.  The store cases at the end need no restatement: they hold the entry to rmpc_timed_plan_device."""
import numpy as np
import pytest

from gpu_support import DEV, _t
from timed_cases import random_case as _random_case
from timed_reference import BAD_ORDER, OUTSIDE, conflicts, store_case
from timed_repair_reference import bay_corridor, repair_ref, two_by_three
from timed_support import goal_index, load_runtime, poisoned, same, stage, workspace

pytestmark = pytest.mark.gpu

PLAN_KEYS = ("paths", "status", "arrive", "key", "best")
KEYS = PLAN_KEYS + ("order_out", "rounds_run", "round_best")


@pytest.fixture(scope="module")
def rt():
    return load_runtime()


def _inputs(rt, grid, starts, goals, orders, movement, occ, stream=None):
    """the device tensors of a case and its fields, as (dict, numpy goal index, numpy goal cells)"""
    goal_cells, gi = goal_index(goals)
    return stage(rt, grid, goal_cells, orders, movement, occ, stream, starts=starts, gi=gi), gi, goal_cells


def _launch_repair(rt, d, T, sep2, rounds, lag, movement, occ, work=None, stream=None):
    """one launch into poisoned outputs -> (the outputs as numpy, the workspace)"""
    torch, lib = rt["torch"], rt["lib"]
    (G, B), (H, W) = d["orders"].shape, d["grid"].shape
    if work is None:
        work = workspace(torch, lib.timed_plan_repair_work_bytes(H, W, T, G, B))
    out = poisoned(torch, KEYS, G, B, T)
    args = lib.timed_repair_args(d["grid"], d["starts"], d["gi"], d["fields"], d["cells"], d["orders"], work, out["paths"],
                                 out["status"], out["arrive"], out["key"], out["best"], out["order_out"], out["rounds_run"],
                                 out["round_best"], rounds, movement=movement, occ_threshold=occ, sep2=sep2, lag=lag)
    lib.timed_plan_repair_device(args, stream=stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, work


def _launch_plan(rt, d, orders, T, sep2, lag, movement, occ):
    """rmpc_timed_plan_device on the same inputs with the device tensor ``orders``"""
    torch, lib = rt["torch"], rt["lib"]
    (G, B), (H, W) = orders.shape, d["grid"].shape
    work = workspace(torch, lib.timed_plan_work_bytes(H, W, T, G))
    out = poisoned(torch, PLAN_KEYS, G, B, T)
    args = lib.timed_plan_args(d["grid"], d["starts"], d["gi"], d["fields"], d["cells"], orders, work, out["paths"],
                               out["status"], out["arrive"], out["key"], out["best"], movement=movement, occ_threshold=occ,
                               sep2=sep2, lag=lag)
    lib.timed_plan_device(args)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _device_repair(rt, grid, starts, goals, orders, T, sep2, rounds, lag=1, movement=4, occ=0.8, stream=None):
    """-> (device results as numpy, the restatement's) for the same fields"""
    d, gi, goal_cells = _inputs(rt, grid, starts, goals, orders, movement, occ, stream)
    got, _ = _launch_repair(rt, d, T, sep2, rounds, lag, movement, occ, stream=stream)
    want = repair_ref(np.asarray(grid, dtype=float), starts, gi, d["fields"].cpu().numpy(), goal_cells, orders, T, sep2, lag,
                      movement, occ, rounds=rounds)
    return got, want


def _same(got, want, keys=KEYS):
    same(got, want, keys)


# ---- against the restatement ----------------------------------------------------------------------------------------------
def test_hand_cases(rt):
    """the cases of tests/test_timed_repair_cpu.py, whose docstrings work them out"""
    g = bay_corridor()
    got, want = _device_repair(rt, g, [7, 13], [13, 7], [[0, 1]], 14, 1, rounds=1)
    _same(got, want)
    assert got["order_out"][0].tolist() == [1, 0] and got["round_best"][0] == 1 and got["rounds_run"][0] == 2
    assert got["status"][0].tolist() == [0, 0]
    assert got["paths"][0, 0].tolist() == [7, 8, 1, 1, 1, 1, 1, 8, 9, 10, 11, 12, 13, 13, 13]
    got, want = _device_repair(rt, g, [7, 13], [13, 7], [[0, 1]], 14, 1, rounds=0)
    _same(got, want)
    assert got["status"][0].tolist() == [0, 5] and got["rounds_run"][0] == 1
    # the 1 x 7 swap fails in every order: R caps the rounds, up to RMPC_TIMED_MAX_ROUNDS, and the tie goes to round 0
    assert rt["lib"].TIMED_MAX_ROUNDS == 16
    for R in (1, 4, 16):
        got, want = _device_repair(rt, np.zeros((1, 7)), [0, 6], [6, 0], [[0, 1], [1, 0]], 8, 1, rounds=R)
        _same(got, want)
        assert got["rounds_run"].tolist() == [R + 1] * 2 and got["round_best"].tolist() == [0, 0]
        assert got["order_out"].tolist() == [[0, 1], [1, 0]]
    # the bad robot is the prefix already
    wall = np.zeros((1, 5))
    wall[0, 3] = 1.0
    got, want = _device_repair(rt, wall, [0, 2], [4, 1], [[0, 1], [1, 0]], 4, 1, rounds=6)
    _same(got, want)
    assert got["rounds_run"].tolist() == [1, 2]
    # a late robot that did not fail is promoted, for the better and for the worse
    got, want = _device_repair(rt, two_by_three(), [5, 3], [4, 2], [[0, 1]], 3, 1, rounds=1)
    _same(got, want)
    assert got["paths"][0].tolist() == [[5, 5, 5, 4], [3, 4, 1, 2]] and got["round_best"][0] == 1
    g = np.ones((3, 7))
    g[1, :] = 0.0
    g[0, 5] = 0.0
    got, want = _device_repair(rt, g, [7, 13], [13, 7], [[0, 1]], 11, 1, rounds=1)
    _same(got, want)
    assert got["round_best"][0] == 0 and got["rounds_run"][0] == 2 and got["arrive"][0].tolist() == [6, 12]


@pytest.mark.parametrize("name,H,W,B,T,G,movement,lag,sep2,R,same_goal", [
    ("small", 7, 5, 3, 9, 2, 4, 1, 2, 2, False),
    ("eight-moves-lag-2", 12, 9, 5, 20, 2, 8, 2, 4, 3, False),
    ("history-in-lds", 65, 70, 6, 40, 2, 8, 1, 5, 1, True),               # two words per row, 256 threads
    ("history-in-the-workspace", 65, 70, 6, 70, 2, 8, 1, 5, 1, True),     # 71 layers of 130 words: beyond the history's LDS
    ("three-words-per-row", 4, 130, 4, 40, 2, 8, 1, 4, 2, False),
    ("128-threads", 100, 20, 4, 30, 2, 4, 3, 10, 2, False),               # 100 words per layer
    ("one-robot", 7, 5, 1, 9, 1, 8, 4, 2, 3, False),
])
def test_repair_is_the_restatement(rt, name, H, W, B, T, G, movement, lag, sep2, R, same_goal):
    g, starts, goals, rng = _random_case(H, W, B, 7 * H + W + T, sep2=sep2)
    if same_goal:                # two robots bound for one cell: whoever is ranked behind is late, in every order
        goals[1] = goals[0]
    orders = [np.arange(B)] + [rng.permutation(B) for _ in range(G - 1)]
    got, want = _device_repair(rt, g, starts, goals, orders, T, sep2, R, lag, movement)
    _same(got, want)
    if same_goal:
        assert max(n[0] for n in want["nbad"]) > 0 and got["rounds_run"].max() == 2
    print(name, "rounds run", got["rounds_run"].tolist(), "best round", got["round_best"].tolist(), "bad", want["nbad"])


@pytest.mark.parametrize("name,H,W,B,G,R,stay", [
    ("two-passes-of-one-wave", 20, 20, 70, 2, 3, False),          # 64 threads: ranks 64 .. 69 are a second pass
    ("five-passes-of-one-wave", 20, 20, 300, 2, 2, False),
    ("five-passes-half-of-them-bad", 20, 20, 300, 1, 2, True),
    ("two-passes-of-two-waves", 100, 20, 200, 1, 1, True),        # 128 threads; the second pass fills one wave and a bit
    ("three-waves-the-last-partly", 65, 65, 130, 1, 1, True),     # 256 threads, 130 ranks, the fourth wave idle
])
def test_partition_across_waves_and_passes(rt, name, H, W, B, G, R, stay):
    """T = 3: most robots cannot arrive and are late.  With ``stay`` every other robot's goal is its start, so that about
    half of the ranks are bad and they interleave with the good ones over the whole order."""
    g, starts, goals, rng = _random_case(H, W, B, H + B, density=0.1, sep2=1)
    if stay:
        goals[::2] = starts[::2]
    orders = [np.arange(B), rng.permutation(B)][2 - G:]
    got, want = _device_repair(rt, g, starts, goals, orders, 3, 1, R)
    _same(got, want)
    for o in range(G):
        bad0 = want["nbad"][o][0]
        assert B // 4 < bad0 < (3 * B // 4 if stay else B) and want["tried"][o][1] != want["tried"][o][0]
        assert sorted(got["order_out"][o].tolist()) == list(range(B))
    print(name, "bad per round", want["nbad"], "best round", got["round_best"].tolist())


def test_rows_that_are_no_permutation(rt):
    g, starts, goals, rng = _random_case(7, 5, 3, 3, sep2=2)
    got, want = _device_repair(rt, g, starts, goals, [[0, 1, 2], [0, 3, 1], [2, 1, 0]], 9, 2, rounds=2)
    _same(got, want)
    assert got["status"][1].tolist() == [BAD_ORDER] * 3 and got["best"][0] in (0, 2)
    assert got["order_out"][1].tolist() == [-1] * 3 and got["rounds_run"][1] == 0 and got["round_best"][1] == -1
    got, want = _device_repair(rt, g, starts, goals, [[1, 1, 0], [-1, 0, 1]], 9, 2, rounds=2)
    _same(got, want)
    assert got["best"][0] == -1 and got["rounds_run"].tolist() == [0, 0] and np.all(got["order_out"] == -1)


def test_skipped_robots_are_never_bad(rt):
    g = np.zeros((7, 7))
    g[:, 4] = 1.0                                      # a wall: columns 5, 6 cannot be reached from the left
    starts, goals = [0, -1, 14, 49], [21, 3, 6, 2]     # robot 1 starts outside, robot 2's goal lies behind the wall,
    got, want = _device_repair(rt, g, starts, goals, [[0, 1, 2, 3], [3, 2, 1, 0]], 12, 2, rounds=3)   # robot 3 past the map
    _same(got, want)
    assert got["status"][0].tolist() == [0, OUTSIDE, 0, OUTSIDE] and want["tried"][0][1] == [2, 0, 1, 3]
    assert want["tried"][1][1] == [2, 3, 1, 0] and got["rounds_run"].tolist() == [2, 2]      # (3 stays behind 2)


def test_side_stream_equals_default_stream(rt):
    torch = rt["torch"]
    g, starts, goals, rng = _random_case(12, 9, 5, 21)
    orders = [np.arange(5), rng.permutation(5)]
    a, want = _device_repair(rt, g, starts, goals, orders, 8, 4, 2, 1, 8)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # (the copies of the inputs run on it too)
        b, _ = _device_repair(rt, g, starts, goals, orders, 8, 4, 2, 1, 8, stream=side.cuda_stream)
    _same(a, want)
    _same(b, a)


# ---- against rmpc_timed_plan_device, on the store ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def store(rt):
    """store_case(16, 0) at G = 4: the inputs on the device, and the repair at R = 0 and R = 2"""
    from robot_mpcs_amd.global_planner import priority_orders
    raw, g_inf, starts, goals = store_case(16, 0, 9)
    orders = priority_orders(16, 4, 0)
    d, gi, goal_cells = _inputs(rt, g_inf, starts, goals, orders, 4, 0.8)
    r0, _ = _launch_repair(rt, d, 128, 9, 0, 1, 4, 0.8)
    r2, work = _launch_repair(rt, d, 128, 9, 2, 1, 4, 0.8)
    return dict(d=d, g_inf=g_inf, starts=starts, goals=goals, orders=orders, r0=r0, r2=r2, work=work)


def test_property_a_without_rounds_it_is_the_plan(rt, store):
    plan = _launch_plan(rt, store["d"], store["d"]["orders"], 128, 9, 1, 4, 0.8)
    _same(store["r0"], plan, PLAN_KEYS)
    assert np.array_equal(store["r0"]["order_out"], store["orders"])
    assert store["r0"]["rounds_run"].tolist() == [1] * 4 and store["r0"]["round_best"].tolist() == [0] * 4


def test_property_b_the_outputs_are_the_plan_of_order_out(rt, store):
    from robot_mpcs_amd.store import STORE
    r2 = store["r2"]
    plan = _launch_plan(rt, store["d"], _t(rt["torch"], r2["order_out"], rt["torch"].int32), 128, 9, 1, 4, 0.8)
    _same(r2, plan, PLAN_KEYS)
    b = int(r2["best"][0])
    assert conflicts(r2["paths"][b], r2["status"][b], STORE.W, 9, 1) == []
    assert np.all(r2["key"] <= store["r0"]["key"])                   # property (c)
    print("store keys, round 0:", store["r0"]["key"].tolist(), "repaired:", r2["key"].tolist(), "rounds", r2["rounds_run"].tolist())


def test_two_runs_on_one_workspace_are_equal(rt, store):
    again, _ = _launch_repair(rt, store["d"], 128, 9, 2, 1, 4, 0.8, work=store["work"])
    _same(again, store["r2"])


def test_timed_routes_with_and_without_repair(rt, store):
    torch = rt["torch"]
    from robot_mpcs_amd.global_planner import TimedRoutes
    tr = TimedRoutes(store["g_inf"], 4, 0.8, 128, 9, lag=1, orders=4, device=DEV, repair=2)
    paths, status, arrive, best = tr.plan(store["starts"], store["goals"])
    torch.cuda.synchronize()
    got = dict(paths=paths, status=status, arrive=arrive, best=best, key=tr.key, order_out=tr.order_out,
               rounds_run=tr.rounds_run, round_best=tr.round_best)
    _same({k: v.cpu().numpy() for k, v in got.items()}, store["r2"])
    plain = TimedRoutes(store["g_inf"], 4, 0.8, 128, 9, lag=1, orders=4, device=DEV)
    paths, status, arrive, best = plain.plan(store["starts"], store["goals"])
    torch.cuda.synchronize()
    got = dict(paths=paths, status=status, arrive=arrive, best=best, key=plain.key)
    _same({k: v.cpu().numpy() for k, v in got.items()}, store["r0"], PLAN_KEYS)
    assert plain.repair == 0 and not hasattr(plain, "order_out")
    assert plain.work.numel() == rt["lib"].timed_plan_work_bytes(*store["g_inf"].shape, 128, 4)
