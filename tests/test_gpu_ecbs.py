"""Focal conflict-based search on the device (rmpc_ecbs_device) against the numpy restatement of
tests/ecbs_reference.py, bit for bit in every output; every launch writes into poisoned outputs and, unless it resumes, a
workspace filled with 0xA5.  The restatement ranks end cells on the fields the device computed, so that both compare the
same doubles.  tests/test_ecbs_cpu.py asserts the outcome of every shared case, so no comparison here is an empty one.
The store with sixteen robots is too slow for the restatement inside a test: there the header's properties are held."""
import math

import numpy as np
import pytest

from cbs_cases import problem
from cbs_reference import BAD_STATE, INF, POOL, ROUNDS, SOLVED
from ecbs_cases import CASES, MANY, STORE4, STORE16
from ecbs_reference import INFO, ecbs_ref
from gpu_support import DEV, _t
from example_loader import load_example
from timed_reference import conflicts, follow_ref, store_case
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
        work = workspace(torch, lib.ecbs_work_bytes(H, W, T, B, c["nodes"], c["expand"]))
    out = {k: v[0] for k, v in poisoned(torch, ("paths", "status", "arrive"), 1, B, T).items()}
    out["info"] = torch.full((lib.ECBS_INFO,), POISON, dtype=torch.int32, device=DEV)
    args = lib.ecbs_args(d["grid"], d["starts"], d["gi"], d["fields"], d["cells"], work, out["paths"], out["status"],
                         out["arrive"], out["info"], c["nodes"], c["expand"], rounds, w=c["w"], resume=resume,
                         movement=c["movement"], occ_threshold=0.8, sep2=c["sep2"], lag=c["lag"])
    lib.ecbs_device(args, stream=stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, work


def _ref(c, d, gi, goal_cells, slices=None):
    return ecbs_ref(c["grid"], c["starts"], gi, d["fields"].cpu().numpy(), goal_cells, c["T"], c["sep2"], c["lag"], c["movement"],
                    nodes=c["nodes"], expand=c["expand"], rounds=c["rounds"], slices=slices, w=c["w"])


def _device(rt, name, stream=None, **over):
    """-> (the case, device results as numpy, the restatement's) for the same fields"""
    c = dict(CASES[name], **over)
    d, gi, goal_cells = _stage(rt, c, stream)
    got, _ = _launch(rt, c, d, c["rounds"], stream=stream)
    return c, got, _ref(c, d, gi, goal_cells)


def _store(k):
    """a store problem of tests/ecbs_cases.py as a case"""
    raw, g, starts, goals = store_case(k["B"], k["seed"], k["sep2"])
    return dict(grid=g, starts=starts, goals=goals, **{n: k[n] for n in ("T", "sep2", "lag", "movement", "nodes", "expand",
                                                                          "rounds", "w")})


# ---- against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_the_search_is_the_restatement(rt, name):
    """at the weights 1, 21/20, 3/2 and 2: the hand cases; 7 x 5 with three robots; 12 x 12 with four, sep2 4, eight moves,
    lag 2; 65 x 70 with the history in LDS (T 40, two nodes per round) and in the workspace (T 70), the cost rows in the
    workspace both times; three words per row; T 1; one robot; a NaN cell; a pool that runs out; rounds that run out; a
    skipped robot; a search that ends without a node"""
    c, got, want = _device(rt, name)
    same(got, want, OUT)
    assert got["info"][0] == c["want"]
    print(name, dict(zip(INFO, got["info"].tolist())), "late", want["late"], "of", want["routes"])


@pytest.mark.parametrize("E", [1, 2, 8])
@pytest.mark.parametrize("name", ["7x5_B3@1_1", "bay@21_20", "65x70_T40@21_20", "12x12_B4@1_1"])
def test_every_batch_size(rt, name, E):
    """one, two and eight nodes per round: the merge of k_ecbs_select takes what the restatement's sort takes"""
    c, got, want = _device(rt, name, expand=E)
    same(got, want, OUT)
    wn, wd = c["w"]
    assert got["info"][0] == SOLVED and got["info"][3] * wd <= wn * got["info"][4]


def test_sixty_four_nodes_per_round(rt):
    """more nodes per round than FOCAL holds in most rounds: the batch is whatever FOCAL has, in the restatement's order"""
    for name in ("65x70_T40@21_20", "4x130@1_1", "bay@1_1"):
        c, got, want = _device(rt, name, expand=64)
        same(got, want, OUT)
        assert got["info"][0] == SOLVED


def test_a_search_with_many_nodes_and_a_selection_in_two_passes(rt):
    """1767 nodes, 64 per round: every thread of the selection holds several ids, and some rounds need its second pass"""
    d, gi, goal_cells = _stage(rt, MANY)
    got, _ = _launch(rt, MANY, d, MANY["rounds"])
    want = _ref(MANY, d, gi, goal_cells)
    same(got, want, OUT)
    assert got["info"][0] == SOLVED and got["info"][5] > 1024 and want["repasses"] >= 1


def test_rounds_that_ran_out_resume_to_the_single_call(rt):
    c = CASES["rounds@21_20"]
    d, gi, goal_cells = _stage(rt, c)
    first, work = _launch(rt, c, d, 7)
    assert first["info"][0] == ROUNDS and first["info"][7] == 7
    same(first, _ref(c, d, gi, goal_cells), OUT)
    mid, work = _launch(rt, c, d, 5, resume=True, work=work)
    same(mid, _ref(c, d, gi, goal_cells, slices=[7, 5]), OUT)
    last, work = _launch(rt, c, d, 4096, resume=True, work=work)
    whole, _ = _launch(rt, dict(c, rounds=4096), d, 4096)
    same(last, whole, OUT)
    same(last, _ref(c, d, gi, goal_cells, slices=[7, 5, 4096]), OUT)
    assert last["info"][0] == SOLVED and first["info"][4] <= mid["info"][4] <= last["info"][4]
    # a solved search resumed stays what it is, and no rounds at all report where it stands
    for rounds in (3, 0):
        again, work = _launch(rt, c, d, rounds, resume=True, work=work)
        assert again["info"][0] == (SOLVED if rounds else ROUNDS)
        same(again, dict(last, info=np.concatenate([again["info"][:1], last["info"][1:]])), OUT)


def test_a_pool_that_ran_out_stops_again_and_a_workspace_without_a_search_is_told_so(rt):
    c = CASES["pool@1_1"]
    d, gi, goal_cells = _stage(rt, c)
    first, work = _launch(rt, c, d, 4096)
    assert first["info"].tolist() == [POOL, 17, 1, 18, 16, 19, 9, 9, 18, 0]
    again, work = _launch(rt, c, d, 4096, resume=True, work=work)
    same(again, first, OUT)
    blank, _ = _launch(rt, c, d, 8, resume=True)                      # (a workspace of 0xA5)
    assert blank["info"].tolist() == [BAD_STATE, -1, 0, INF, INF, 0, 0, 0, INF, 0]
    assert np.all(blank["paths"] == -1) and blank["arrive"].tolist() == [13, 13] and blank["status"].tolist() == [0, 0]
    other, _ = _launch(rt, dict(c, w=(21, 20)), d, 8, resume=True, work=work)      # the search of another weight
    assert other["info"][0] == BAD_STATE


def test_side_stream_and_two_plans_on_one_workspace(rt):
    torch = rt["torch"]
    c, a, want = _device(rt, "12x12_B4@21_20")
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # (the copies of the inputs run on it too)
        _, b, _ = _device(rt, "12x12_B4@21_20", stream=side.cuda_stream)
    same(a, want, OUT)
    same(b, a, OUT)
    d, gi, goal_cells = _stage(rt, c)
    first, work = _launch(rt, c, d, c["rounds"])
    second, _ = _launch(rt, c, d, c["rounds"], work=work)
    same(first, a, OUT)
    same(second, a, OUT)


def test_the_store_with_four_robots_is_the_restatement(rt):
    """41 x 41 at T 128: the history and the cost rows in LDS"""
    c = _store(STORE4)
    d, gi, goal_cells = _stage(rt, c)
    got, _ = _launch(rt, c, d, c["rounds"])
    want = _ref(c, d, gi, goal_cells)
    same(got, want, OUT)
    assert got["info"][0] == SOLVED and got["info"][6] == STORE4["expansions"] and want["late"] >= 1
    print(dict(zip(INFO, got["info"].tolist())))


# ---- the fleet -------------------------------------------------------------------------------------------------------------
def test_the_store_with_sixteen_robots_is_planned_within_a_tenth_of_the_optimum(rt):
    """w = 11/10, one node per round, the budget of tests/ecbs_cases.py: SOLVED, no conflict, cost * 10 <= 11 * bound,
    the bound no lower than the root of rmpc_cbs_device, the cost no higher than the best of 16 repaired prioritised
    orders; then 40 scripted follower steps on the plan, every step the restatement's."""
    torch, lib = rt["torch"], rt["lib"]
    from robot_mpcs_amd.global_planner import TimedFollower, TimedRoutes
    c = _store(STORE16)
    B, T, (H, W) = 16, c["T"], c["grid"].shape
    d, gi, goal_cells = _stage(rt, c)
    got, _ = _launch(rt, c, d, c["rounds"])
    info = dict(zip(INFO, got["info"].tolist()))
    print(info)
    assert info["outcome"] == SOLVED and info["conflict_free"] == 1 and info["nconf"] == 0
    assert conflicts(got["paths"], got["status"], W, c["sep2"], c["lag"]) == []
    assert info["cost"] * 10 <= 11 * info["bound"] and info["cost"] == int(got["arrive"].sum())
    # the root of plain conflict-based search: every robot's least arrive
    out = {k: v[0] for k, v in poisoned(torch, ("paths", "status", "arrive"), 1, B, T).items()}
    root = torch.full((lib.CBS_INFO,), POISON, dtype=torch.int32, device=DEV)
    lib.cbs_device(lib.cbs_args(d["grid"], d["starts"], d["gi"], d["fields"], d["cells"],
                                workspace(torch, lib.cbs_work_bytes(H, W, T, B, 16, 1)), out["paths"], out["status"],
                                out["arrive"], root, 16, 1, 0, movement=4, occ_threshold=0.8, sep2=c["sep2"], lag=c["lag"]))
    tr = TimedRoutes(d["grid"], 4, 0.8, T, c["sep2"], lag=c["lag"], orders=16, seed=0, device=DEV, repair=3)
    t_paths, t_status, t_arrive, t_best = tr.plan(_t(torch, np.asarray(c["starts"]), torch.int32),
                                                  _t(torch, np.asarray(c["goals"]), torch.int32))
    torch.cuda.synchronize()
    root_cost = int(root[lib.CBS_COST].item())
    b = int(t_best.item())
    assert b >= 0 and bool((t_status[b] <= 0).all().item())
    prioritised = int(t_arrive[b].sum().item())
    print("root", root_cost, "bound", info["bound"], "cost", info["cost"], "prioritised", prioritised)
    assert info["bound"] >= root_cost
    assert info["cost"] <= prioritised

    paths = got["paths"]
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
    assert idx.max() >= 20


def test_bounded_timed_routes_against_the_calls_by_hand(rt):
    torch, lib = rt["torch"], rt["lib"]
    from robot_mpcs_amd.global_planner import BoundedTimedRoutes
    c = CASES["12x12_B4@21_20"]
    d, gi, goal_cells = _stage(rt, c)
    whole, _ = _launch(rt, c, d, 4096)
    part, _ = _launch(rt, c, d, 2)
    btr = BoundedTimedRoutes(c["grid"], c["movement"], 0.8, c["T"], c["sep2"], w=c["w"], lag=c["lag"], nodes=c["nodes"],
                             expand=c["expand"], rounds=2, device=DEV)
    paths, status, arrive, info = btr.plan(c["starts"], c["goals"])
    torch.cuda.synchronize()
    same({k: v.cpu().numpy() for k, v in dict(paths=paths, status=status, arrive=arrive, info=info).items()}, part, OUT)
    assert np.array_equal(btr.fields.cpu().numpy(), d["fields"].cpu().numpy())
    paths, status, arrive, info = btr.more(4096)
    gap, ratio = btr.gap(arrive + 1), btr.ratio()
    torch.cuda.synchronize()
    same({k: v.cpu().numpy() for k, v in dict(paths=paths, status=status, arrive=arrive, info=info).items()}, whole, OUT)
    assert part["info"][0] == ROUNDS and whole["info"][0] == SOLVED
    cost, bound = int(whole["info"][3]), int(whole["info"][4])
    assert ratio.cpu().tolist() == [cost, bound] and ratio.is_cuda and cost * 20 <= 21 * bound
    assert gap.cpu().tolist() == [cost + 4 - bound, 4]
    assert btr.work.numel() == lib.ecbs_work_bytes(12, 12, c["T"], 4, c["nodes"], c["expand"])


# ---- closed loop -------------------------------------------------------------------------------------------------------
def test_closed_loop_on_the_searched_plan(rt):
    """examples/fleet_store_bounded.py, sixteen boxers on store seed 0: the search ends SOLVED within 11/10 of its bound
    and no worse than the repaired prioritised plan, the fleet follows the searched plan, and the run meets the gates of
    the timed run: every robot arrives, no pair of robots closer than r_i + r_j - 1e-3 m, no failed solve."""
    ex = load_example("fleet_store_bounded")
    r = ex.run(B=ex.ROBOTS, steps=220, seed=0)
    print(r)
    assert r["outcome"] == SOLVED and r["conflict_free"] == 1 and r["followed"] == "searched", r
    assert r["cost"] * 10 <= 11 * r["bound"] and r["ratio"] <= 1.1, r
    assert r["prioritised_sum"] is None or r["prioritised_sum"] >= r["cost"], r
    assert r["arrivals"] == ex.ROBOTS, r
    assert r["min_pair_gap_m"] >= -1e-3, r
    assert r["failed_share"] == 0.0, r
