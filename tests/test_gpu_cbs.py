"""Conflict-based search on the device (rmpc_cbs_device) against the numpy restatement of
tests/cbs_reference.py, bit for bit in every output; every launch writes into poisoned outputs and, unless it resumes, a
workspace filled with 0xA5.  The restatement ranks end cells on the fields the device computed, so that both compare the
same doubles.  tests/test_cbs_cpu.py asserts the outcome of every shared case, so no comparison here is an empty one."""
import math

import numpy as np
import pytest

from cbs_cases import CASES, problem
from cbs_reference import BAD_STATE, INF, INFO, POOL, ROUNDS, SOLVED, cbs_ref
from gpu_support import DEV, _t
from example_loader import load_example
from timed_reference import conflicts, follow_ref
from timed_support import POISON, load_runtime, poisoned, same, stage, workspace

pytestmark = pytest.mark.gpu

OUT = ("paths", "status", "arrive", "info")


@pytest.fixture(scope="module")
def rt():
    return load_runtime()


def _stage(rt, c, stream=None):
    goal_cells, gi = problem(c)
    return stage(rt, c["grid"], goal_cells, [[0]], c["movement"], 0.8, stream, starts=c["starts"], gi=gi), gi, goal_cells


def _launch(rt, c, d, rounds, resume=False, work=None, stream=None):
    """one call into poisoned outputs -> (the outputs as numpy, the workspace)"""
    torch, lib = rt["torch"], rt["lib"]
    B, T, (H, W) = len(c["starts"]), c["T"], c["grid"].shape
    if work is None:
        work = workspace(torch, lib.cbs_work_bytes(H, W, T, B, c["nodes"], c["expand"]))
    out = {k: v[0] for k, v in poisoned(torch, ("paths", "status", "arrive"), 1, B, T).items()}
    out["info"] = torch.full((lib.CBS_INFO,), POISON, dtype=torch.int32, device=DEV)
    args = lib.cbs_args(d["grid"], d["starts"], d["gi"], d["fields"], d["cells"], work, out["paths"], out["status"],
                        out["arrive"], out["info"], c["nodes"], c["expand"], rounds, resume=resume, movement=c["movement"],
                        occ_threshold=0.8, sep2=c["sep2"], lag=c["lag"])
    lib.cbs_device(args, stream=stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, work


def _ref(c, d, gi, goal_cells, slices=None):
    return cbs_ref(c["grid"], c["starts"], gi, d["fields"].cpu().numpy(), goal_cells, c["T"], c["sep2"], c["lag"], c["movement"],
                   nodes=c["nodes"], expand=c["expand"], rounds=c["rounds"], slices=slices)


def _device(rt, name, stream=None, **over):
    """-> (the case, device results as numpy, the restatement's) for the same fields"""
    c = dict(CASES[name], **over)
    d, gi, goal_cells = _stage(rt, c, stream)
    got, _ = _launch(rt, c, d, c["rounds"], stream=stream)
    return c, got, _ref(c, d, gi, goal_cells)


# ---- against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_the_search_is_the_restatement(rt, name):
    """the hand cases; 7 x 5 with three robots; 12 x 12 with four, sep2 4, eight moves, lag 2; 65 x 70 with the history in
    LDS (T 40, two nodes per round) and in the workspace (T 70); three words per row; T 1; one robot; a NaN cell; a pool
    that runs out; rounds that run out; a skipped robot; a search that ends without a node"""
    c, got, want = _device(rt, name)
    same(got, want, OUT)
    assert got["info"][0] == c["want"]
    print(name, dict(zip(INFO, got["info"].tolist())))


@pytest.mark.parametrize("E", [1, 2, 8])
@pytest.mark.parametrize("name", ["7x5_B3", "bay"])
def test_every_batch_size(rt, name, E):
    c, got, want = _device(rt, name, expand=E)
    same(got, want, OUT)
    assert got["info"][0] == SOLVED and got["info"][3] == _device(rt, name)[1]["info"][3]


def test_rounds_that_ran_out_resume_to_the_single_call(rt):
    c = CASES["rounds"]
    d, gi, goal_cells = _stage(rt, c)
    first, work = _launch(rt, c, d, 7)
    assert first["info"].tolist() == [ROUNDS, 10, 0, 15, 15, 15, 7, 7]
    same(first, _ref(c, d, gi, goal_cells), OUT)
    mid, work = _launch(rt, c, d, 5, resume=True, work=work)
    same(mid, _ref(c, d, gi, goal_cells, slices=[7, 5]), OUT)
    last, work = _launch(rt, c, d, 4096, resume=True, work=work)
    whole, _ = _launch(rt, dict(c, rounds=4096), d, 4096)
    same(last, whole, OUT)
    same(last, _ref(c, d, gi, goal_cells, slices=[7, 5, 4096]), OUT)
    assert last["info"].tolist() == [SOLVED, 48, 1, 18, 18, 53, 26, 26] and first["info"][4] <= mid["info"][4] <= last["info"][4]
    # a solved search resumed stays what it is, and no rounds at all report where it stands
    for rounds in (3, 0):
        again, work = _launch(rt, c, d, rounds, resume=True, work=work)
        assert again["info"][0] == (SOLVED if rounds else ROUNDS)
        same(again, dict(last, info=np.concatenate([again["info"][:1], last["info"][1:]])), OUT)


def test_a_pool_that_ran_out_stops_again_and_a_workspace_without_a_search_is_told_so(rt):
    c = CASES["pool"]
    d, gi, goal_cells = _stage(rt, c)
    first, work = _launch(rt, c, d, 4096)
    assert first["info"].tolist() == [POOL, 5, 0, 16, 16, 19, 9, 9]
    again, work = _launch(rt, c, d, 4096, resume=True, work=work)
    same(again, first, OUT)
    blank, _ = _launch(rt, c, d, 8, resume=True)                      # (a workspace of 0xA5)
    assert blank["info"].tolist() == [BAD_STATE, -1, 0, INF, INF, 0, 0, 0]
    assert np.all(blank["paths"] == -1) and blank["arrive"].tolist() == [13, 13] and blank["status"].tolist() == [0, 0]
    other, _ = _launch(rt, dict(c, sep2=2), d, 8, resume=True, work=work)      # the search of other rules
    assert other["info"][0] == BAD_STATE


def test_side_stream_and_two_plans_on_one_workspace(rt):
    torch = rt["torch"]
    c, a, want = _device(rt, "12x12_B4")
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # (the copies of the inputs run on it too)
        _, b, _ = _device(rt, "12x12_B4", stream=side.cuda_stream)
    same(a, want, OUT)
    same(b, a, OUT)
    d, gi, goal_cells = _stage(rt, c)
    first, work = _launch(rt, c, d, c["rounds"])
    second, _ = _launch(rt, c, d, c["rounds"], work=work)
    same(first, a, OUT)
    same(second, a, OUT)


# ---- against the prioritised plan and the follower ------------------------------------------------------------------------
def test_property_c_against_the_timed_plan_and_the_follower_takes_the_plan(rt):
    """12 x 12 with four robots: every failure-free order of rmpc_timed_plan_device itself sums to at least the proven
    cost; the reported plan then goes through ``TimedFollower`` for 40 scripted steps (each robot moves 0.8 of the way
    to its goal, robot 1 stands still for the first 10), every step the restatement's."""
    import itertools
    torch, lib = rt["torch"], rt["lib"]
    from robot_mpcs_amd.global_planner import TimedFollower
    c, got, want = _device(rt, "12x12_B4")
    same(got, want, OUT)
    assert got["info"][0] == SOLVED and got["info"][2] == 1
    d, gi, goal_cells = _stage(rt, c)
    orders = np.array(list(itertools.permutations(range(4))), np.int32)
    G, B, T, (H, W) = len(orders), 4, c["T"], c["grid"].shape
    out = poisoned(torch, ("paths", "status", "arrive", "key", "best"), G, B, T)
    args = lib.timed_plan_args(d["grid"], d["starts"], d["gi"], d["fields"], d["cells"], _t(torch, orders, torch.int32),
                               workspace(torch, lib.timed_plan_work_bytes(H, W, T, G)), out["paths"], out["status"],
                               out["arrive"], out["key"], out["best"], movement=c["movement"], occ_threshold=0.8,
                               sep2=c["sep2"], lag=c["lag"])
    lib.timed_plan_device(args)
    torch.cuda.synchronize()
    status, arrive = out["status"].cpu().numpy(), out["arrive"].cpu().numpy()
    clean = np.all(status <= 0, axis=1)
    assert clean.sum() >= 1
    sums = arrive[clean].sum(axis=1)
    assert sums.min() >= got["info"][3] == got["info"][4]
    print("cost", got["info"][3], "failure-free orders", int(clean.sum()), "their sums", sorted(set(sums.tolist())))

    paths = got["paths"]
    assert conflicts(paths, got["status"], W, c["sep2"], c["lag"]) == []
    fol = TimedFollower(_t(torch, paths, torch.int32), W, 0.0, 0.0, 1.0, 0.3, c["sep2"], c["lag"])
    starts = np.asarray(c["starts"])
    pos = np.stack([(starts % W).astype(float), (starts // W).astype(float), np.zeros(B)], 1)
    goal = np.full((B, 3), math.nan)
    idx = np.zeros(B, np.int32)
    d_goal = _t(torch, goal)
    for step in range(40):
        idx, goal, blk = follow_ref(paths, idx, pos, goal, W, 0.0, 0.0, 1.0, 0.3, c["sep2"], c["lag"])
        fol.step(_t(torch, pos), d_goal)
        torch.cuda.synchronize()
        assert np.array_equal(fol.idx.cpu().numpy(), idx), step
        assert np.array_equal(d_goal.cpu().numpy(), goal), step
        assert np.array_equal(fol.blocked.cpu().numpy(), blk), step
        move = np.full((B, 1), 0.8)
        if step < 10:
            move[1] = 0.0
        pos[:, :2] += move * (goal[:, :2] - pos[:, :2])
    assert idx.max() >= got["arrive"].max() - 1


def test_optimal_timed_routes_against_the_calls_by_hand(rt):
    torch, lib = rt["torch"], rt["lib"]
    from robot_mpcs_amd.global_planner import OptimalTimedRoutes
    c = CASES["12x12_B4"]
    d, gi, goal_cells = _stage(rt, c)
    whole, _ = _launch(rt, c, d, 4096)
    part, _ = _launch(rt, c, d, 2)
    otr = OptimalTimedRoutes(c["grid"], c["movement"], 0.8, c["T"], c["sep2"], lag=c["lag"], nodes=c["nodes"],
                             expand=c["expand"], rounds=2, device=DEV)
    paths, status, arrive, info = otr.plan(c["starts"], c["goals"])
    torch.cuda.synchronize()
    same({k: v.cpu().numpy() for k, v in dict(paths=paths, status=status, arrive=arrive, info=info).items()}, part, OUT)
    assert np.array_equal(otr.fields.cpu().numpy(), d["fields"].cpu().numpy())
    paths, status, arrive, info = otr.more(4096)
    gap = otr.gap(arrive + 1)
    torch.cuda.synchronize()
    same({k: v.cpu().numpy() for k, v in dict(paths=paths, status=status, arrive=arrive, info=info).items()}, whole, OUT)
    assert gap.cpu().tolist() == [len(c["starts"])] * 2 and part["info"][0] == ROUNDS and whole["info"][0] == SOLVED
    assert otr.work.numel() == lib.cbs_work_bytes(12, 12, c["T"], 4, c["nodes"], c["expand"])


# ---- closed loop -------------------------------------------------------------------------------------------------------
def test_closed_loop_on_the_optimal_plan(rt):
    """examples/fleet_store_optimal.py at its own fleet size on store seed 0, a short run: the search must end SOLVED
    with cost >= bound, and the run meets the gates of the timed run of tests/test_gpu_timed.py: at most 1 % of the
    robot-steps failed, no pair of robots closer than r_i + r_j - 1e-3 m."""
    ex = load_example("fleet_store_optimal")
    r = ex.run(B=ex.ROBOTS, steps=120, seed=0)
    print(r)
    assert r["outcome"] == SOLVED and r["conflict_free"] == 1 and r["cost"] == r["bound"], r
    assert r["prioritised_sum"] is None or r["prioritised_sum"] >= r["cost"], r
    assert r["failed_share"] <= 0.01, r
    assert r["min_pair_gap_m"] >= -1e-3, r
