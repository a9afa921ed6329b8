"""Tours of several tasks per robot on the device (rmpc_tours_device, rmpc_follow_tour_device, include/rmpc_tours.h,
DESIGN.md 24) against the restatements of tests/tours_reference.py, bit for bit in every output: both modes, with and
without holes, several problems in one call, poisoned buffers, NULL outputs, stream order, the scale; the follower on
constructed indices and through scripted steps; TourPlanner against the composed restatements of the planner; one closed
loop of 16 boxers through 24 picks."""
import math

import numpy as np
import pytest

from gpu_support import DEV, _t
from tours_cases import KINDS, make_problem, store_draw
from tours_reference import follow_tour_ref, plan_ref, tours_problem_ref

pytestmark = pytest.mark.gpu

INF, NAN = math.inf, math.nan
REFS = {}
OUTS = ("tours", "len", "cost", "owner", "count", "total", "span", "build_steps", "rounds")


@pytest.fixture(scope="module")
def rt():
    import torch
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return dict(torch=torch, lib=_lib)


def ref_of(kind, B, T, K, mode, holes, scale=1024.0, max_rounds=1 << 30):
    """(start_cost, task_cost, restatement's report), computed once per case and left unchanged"""
    key = (kind, B, T, K, mode, holes, scale, max_rounds)
    if key not in REFS:
        s, d = make_problem(kind, B, T, holes)
        s.setflags(write=False)
        d.setflags(write=False)
        REFS[key] = (s, d, tours_problem_ref(s, d, K, mode, scale, max_rounds))
    return REFS[key]


def run(rt, s, d, K, mode, scale=1024.0, max_rounds=1 << 30, poison=-77, outputs=True, stream=None):
    """one call into poisoned outputs and a poisoned workspace: the outputs as a dict of numpy arrays (G leading when
    the costs have it), None for those not asked for"""
    torch, lib = rt["torch"], rt["lib"]
    s, d = np.asarray(s), np.asarray(d)
    lead = s.shape[:-2]
    G = 1 if not lead else lead[0]
    B, T = s.shape[-2:]
    ts, td = _t(torch, s), _t(torch, d)
    full = lambda shape, dt: torch.full(shape, poison, dtype=dt, device=DEV)
    tours, lens, cost = full(lead + (B, K), torch.int32), full(lead + (B,), torch.int32), full(lead + (B,), torch.int64)
    opt = dict(owner=full(lead + (T,), torch.int32), count=full((G,), torch.int32), total=full((G,), torch.int64),
               span=full((G,), torch.int64), build_steps=full((G,), torch.int32), rounds=full((G,), torch.int32)) if outputs else {}
    work = torch.full((lib.tours_work_bytes(G, B, T),), poison & 0xFF, dtype=torch.uint8, device=DEV)
    lib.tours_device(ts, td, tours, lens, cost, mode, scale, max_rounds, work=work, stream=stream, **opt)
    assert np.array_equal(ts.cpu().numpy(), s, equal_nan=True) and np.array_equal(td.cpu().numpy(), d, equal_nan=True)
    out = dict(tours=tours, len=lens, cost=cost, **opt)
    return {k: out[k].cpu().numpy() if k in out else None for k in OUTS}


def same(got, want, g=None):
    for key in OUTS:
        have = got[key] if g is None else got[key][g]
        if key in ("count", "total", "span", "build_steps", "rounds") and g is None:
            have = have[0]
        assert np.array_equal(have, want[key]), (key, have, want[key])


# the shapes that can break the kernel: the least problem, one tour, room in the tours (relocations between them), every
# tour full (only exchanges between tours), more robots than tasks, a wave boundary, more waves and uneven tails, the
# robot limit
SHAPES = [(1, 1, 1), (1, 7, 7), (3, 7, 3), (2, 6, 3), (5, 3, 1), (9, 64, 8), (9, 65, 8), (17, 130, 9), (40, 257, 7), (1024, 33, 1)]


@pytest.mark.parametrize("B,T,K", SHAPES)
@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_device_is_the_restatement(rt, kind, mode, holes, B, T, K):
    s, d, want = ref_of(kind, B, T, K, mode, holes)
    same(run(rt, s, d, K, mode), want)
    if holes:
        assert want["count"] < T and (want["owner"] == -1).any()         # the task no edge leads to
    else:
        assert want["count"] == min(T, B * K)


def test_the_shapes_reach_relocations_exchanges_and_full_tours():
    """what SHAPES is there to reach, on the restatement: rounds are taken; with (2, 6, 3) every tour is full"""
    assert sum(ref_of(k, 3, 7, 3, m, False)[2]["rounds"] for k in KINDS for m in (0, 1)) > 0
    assert sum(ref_of(k, 2, 6, 3, m, False)[2]["rounds"] for k in KINDS for m in (0, 1)) > 0
    assert all((ref_of(k, 2, 6, 3, m, False)[2]["len"] == 3).all() for k in KINDS for m in (0, 1))
    assert ref_of("grid", 40, 257, 7, 1, False)[2]["rounds"] > 20


@pytest.mark.parametrize("mode", [0, 1])
def test_device_is_the_restatement_at_the_task_limit(rt, mode):
    """(64, 1024, 16): 1024 threads, every tour full after the build; three rounds keep the restatement within seconds"""
    s, d, want = ref_of("grid", 64, 1024, 16, mode, False, max_rounds=3)
    same(run(rt, s, d, 16, mode, max_rounds=3), want)
    assert want["count"] == 1024 and want["rounds"] == 3


def test_max_rounds_zero_and_a_cap(rt):
    s, d, free = ref_of("grid", 17, 130, 9, 1, False)
    assert free["rounds"] > 5
    for cap in (0, 1, 5):
        want = tours_problem_ref(s, d, 9, 1, max_rounds=cap)
        assert want["rounds"] == cap
        same(run(rt, s, d, 9, 1, max_rounds=cap), want)


def test_all_untakeable_problems(rt):
    for B, T, K, value in ((9, 4, 2, INF), (3, 70, 5, NAN), (130, 2, 1, -1.0), (4, 65, 65, 1e9)):
        s, d = np.full((B, T), value), np.ones((T, T))
        for mode in (0, 1):
            got = run(rt, s, d, K, mode)
            assert (got["tours"] == -1).all() and (got["len"] == 0).all() and (got["cost"] == 0).all()
            assert (got["owner"] == -1).all()
            assert [int(got[k][0]) for k in ("count", "total", "span", "build_steps", "rounds")] == [0] * 5
            same(got, tours_problem_ref(s, d, K, mode))


def test_three_problems_in_one_call_are_the_three_lone_calls(rt):
    """G = 3 problems with hole patterns of their own; NULL optional outputs change nothing else; a second poison changes
    nothing"""
    for B, T, K in ((3, 7, 3), (9, 65, 8), (17, 130, 9)):
        probs = [make_problem(k, B, T, h) for k, h in (("unif", True), ("ties", False), ("grid", True))]
        s, d = np.stack([p[0] for p in probs]), np.stack([p[1] for p in probs])
        for mode in (0, 1):
            got = run(rt, s, d, K, mode)
            for g in range(3):
                want = tours_problem_ref(s[g], d[g], K, mode)
                same(got, want, g)
                same(run(rt, s[g], d[g], K, mode, poison=123456), want)
            bare = run(rt, s, d, K, mode, poison=5, outputs=False)
            assert all(np.array_equal(bare[k], got[k]) for k in ("tours", "len", "cost")) and bare["owner"] is None


def test_calls_on_a_side_stream_see_their_producer(rt):
    """the costs are written by a kernel on the side stream just ahead of each call, into buffers that held other costs;
    the workspace is shared by the two calls; the result is the default stream's"""
    torch, lib = rt["torch"], rt["lib"]
    B, T, K = 17, 130, 9
    first, second = make_problem("unif", B, T, True), make_problem("grid", B, T, False)
    want = [tours_problem_ref(*first, K, 1), tours_problem_ref(*second, K, 1)]
    assert not np.array_equal(want[0]["tours"], want[1]["tours"])
    same(run(rt, *first, K, 1), want[0])
    src = [(_t(torch, s), _t(torch, d)) for s, d in (first, second)]
    work = torch.zeros(lib.tours_work_bytes(1, B, T), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(device=0)
    for _ in range(3):
        s = torch.full((B, T), NAN, dtype=torch.float64, device=DEV)
        d = torch.full((T, T), NAN, dtype=torch.float64, device=DEV)
        outs = []
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for ss, dd in src:
                s.copy_(ss * 1.0)                                          # the producers
                d.copy_(dd * 1.0)
                o = dict(tours=torch.full((B, K), -5, dtype=torch.int32, device=DEV), len=torch.zeros(B, dtype=torch.int32, device=DEV),
                         cost=torch.zeros(B, dtype=torch.int64, device=DEV), owner=torch.zeros(T, dtype=torch.int32, device=DEV),
                         count=torch.zeros(1, dtype=torch.int32, device=DEV), total=torch.zeros(1, dtype=torch.int64, device=DEV),
                         span=torch.zeros(1, dtype=torch.int64, device=DEV), build_steps=torch.zeros(1, dtype=torch.int32, device=DEV),
                         rounds=torch.zeros(1, dtype=torch.int32, device=DEV))
                lib.tours_device(s, d, o["tours"], o["len"], o["cost"], 1, 1024.0, 1 << 30, o["owner"], o["count"], o["total"],
                                 o["span"], o["build_steps"], o["rounds"], work, stream=side.cuda_stream)
                outs.append(o)
        side.synchronize()
        for o, w in zip(outs, want):
            same({k: v.cpu().numpy() for k, v in o.items()}, w)


def test_scale_changes_q_as_the_restatement_says(rt):
    s, d, want = ref_of("grid", 9, 65, 8, 0, False)
    coarse = tours_problem_ref(s, d, 8, 0, scale=1.0)
    same(run(rt, s, d, 8, 0, scale=1.0), coarse)
    assert coarse["total"] != want["total"] and not np.array_equal(coarse["cost"] * 1024, want["cost"])


# ---- the follower -----------------------------------------------------------------------------------------------------
def follow(rt, paths, lens, idx, pos, stop_at, leg, served, now, threshold=1.3, stop_tol=0.3, W=41, stride_pad=0):
    """one device call on copies: (goal, idx, leg, served) as numpy; goal rows of robots without a path keep -5"""
    torch, lib = rt["torch"], rt["lib"]
    B = len(lens)
    wide = np.full((B, pos.shape[1] + stride_pad), 99.0)
    wide[:, :pos.shape[1]] = pos
    tp = _t(torch, wide)[:, :pos.shape[1]] if stride_pad else _t(torch, pos)
    t = dict(paths=_t(torch, paths, torch.int32), lens=_t(torch, lens, torch.int32), idx=_t(torch, idx, torch.int32),
             stop_at=_t(torch, stop_at, torch.int32), leg=_t(torch, leg, torch.int32), served=_t(torch, served, torch.int32))
    goal = torch.full((B, 3), -5.0, dtype=torch.float64, device=DEV)
    lib.follow_tour_device(t["paths"], t["lens"], t["idx"], tp, goal, W, -9.0, -9.0, 0.45, threshold, t["stop_at"], t["leg"],
                           t["served"], now, stop_tol)
    assert np.array_equal(t["paths"].cpu().numpy(), paths) and np.array_equal(t["stop_at"].cpu().numpy(), stop_at)
    return goal.cpu().numpy(), t["idx"].cpu().numpy(), t["leg"].cpu().numpy(), t["served"].cpu().numpy()


def follow_ref(paths, lens, idx, pos, stop_at, leg, served, now, threshold=1.3, stop_tol=0.3, W=41):
    idx, leg, served = idx.copy(), leg.copy(), served.copy()
    goal = follow_tour_ref(paths, lens, idx, pos, W, -9.0, -9.0, 0.45, threshold, stop_at, leg, served, now, stop_tol)
    return np.where(np.isnan(goal), -5.0, goal), idx, leg, served


def test_follower_on_constructed_indices(rt):
    """a stop on the last cell, two stops at one index, leg == K, len == 0, a waypoint that is no stop -- each near enough
    and not; positions with the stride of a wider tensor"""
    W, K = 41, 3
    path = np.array([5 * W + 5, 5 * W + 6, 5 * W + 7, 6 * W + 8, 7 * W + 8, 8 * W + 8], dtype=np.int32)
    cases = []                                                             # (len, idx, leg, stop_at, offset to the cell)
    for off in (0.0, 0.29, 0.31, 1.29, 1.31):
        cases += [(6, 5, 2, [1, 3, 5], off), (6, 5, 3, [1, 3, 5], off),    # the last cell: a stop / all served
                  (6, 3, 0, [3, 3, 5], off), (6, 3, 1, [3, 3, 5], off),    # two stops at one index: the first, the second
                  (6, 3, 2, [3, 3, 3], off), (6, 2, 1, [0, 4, -1], off),   # the last of three; no stop here
                  (6, 4, 1, [0, 4, -1], off), (6, 4, 2, [0, 4, -1], off),  # a stop; past the last used entry
                  (0, 2, 0, [1, 3, 5], off), (-3, 2, 0, [1, 3, 5], off),   # no path: nothing moves
                  (6, 9, 0, [1, 3, 5], off), (6, -2, -1, [0, 3, 5], off),  # idx and leg outside their range
                  (1, 0, 0, [0, -1, -1], off), (1, 0, 0, [0, 0, 0], off)]
    B = len(cases)
    paths = np.tile(path, (B, 1))
    lens = np.array([c[0] for c in cases], dtype=np.int32)
    idx = np.array([c[1] for c in cases], dtype=np.int32)
    leg = np.array([c[2] for c in cases], dtype=np.int32)
    stop_at = np.array([c[3] for c in cases], dtype=np.int32)
    at = paths[np.arange(B), np.clip(idx, 0, np.maximum(lens, 1) - 1)]
    pos = np.stack([-9.0 + (at % W) * 0.45 + np.array([c[4] for c in cases]), -9.0 + (at // W) * 0.45], 1)
    served = np.full((B, K), -1, dtype=np.int32)
    want = follow_ref(paths, lens, idx, pos, stop_at, leg, served, 17)
    assert (want[3] == 17).sum() >= 8 and (want[1] != np.clip(idx, 0, 5)).sum() >= 8
    for pad in (0, 5):
        got = follow(rt, paths, lens, idx, pos, stop_at, leg, served, 17, stride_pad=pad)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (g, w)


def test_follower_through_forty_scripted_steps(rt):
    """70 robots (more than one wave) walk towards their goals 0.3 m per step on random paths with random stops; idx, leg,
    served and goal equal the restatement's after every step"""
    rng = np.random.default_rng(31)
    B, K, L, W = 70, 4, 30, 41
    r0, c0 = rng.integers(2, 8, B), rng.integers(2, 8, B)
    steps = rng.integers(0, 2, size=(B, L, 2))
    cells = np.stack([r0[:, None] + np.cumsum(steps[:, :, 0], 1), c0[:, None] + np.cumsum(steps[:, :, 1], 1)], 2)
    paths = (cells[:, :, 0] * W + cells[:, :, 1]).astype(np.int32)
    lens = rng.integers(1, L + 1, B).astype(np.int32)
    lens[::9] = 0
    stop_at = np.sort(rng.integers(0, L, size=(B, K)), 1).astype(np.int32)
    stop_at = np.where(stop_at < np.maximum(lens, 1)[:, None], stop_at, -1).astype(np.int32)
    stop_at = np.where(np.cumsum(stop_at < 0, 1) > 0, -1, stop_at).astype(np.int32)
    idx, leg, served = np.zeros(B, np.int32), np.zeros(B, np.int32), np.full((B, K), -1, np.int32)
    pos = np.stack([-9.0 + (paths[:, 0] % W) * 0.45, -9.0 + (paths[:, 0] // W) * 0.45], 1) + rng.uniform(-0.2, 0.2, (B, 2))
    for now in range(40):
        want = follow_ref(paths, lens, idx, pos, stop_at, leg, served, now, threshold=0.8, stop_tol=0.2)
        got = follow(rt, paths, lens, idx, pos, stop_at, leg, served, now, threshold=0.8, stop_tol=0.2)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), now
        goal, idx, leg, served = want
        d = np.where(lens[:, None] > 0, goal[:, :2] - pos, 0.0)
        pos = pos + d * np.minimum(1.0, 0.3 / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12))
    assert (served >= 0).sum() > 40 and (leg > 1).sum() > 10


# ---- TourPlanner --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["span", "sum"])
def test_tour_planner_is_the_composed_restatement(rt, mode):
    """the 41 x 41 store, 16 robots, 24 picks, K = 2: fields, both cost matrices, the tours and every output of the
    rule, the joined routes and stop_at equal field_ref -> route_costs_ref -> the restatement -> descend_ref; every
    route is contiguous under the movement; stop_at points at the picks' cells"""
    torch = rt["torch"]
    from robot_mpcs_amd.global_planner import TourFollower, TourPlanner
    from robot_mpcs_amd.store import STORE as S
    data, starts, goals = store_draw(16, 24, seed=0)
    want = plan_ref(data, starts, goals, 2, mode=dict(sum=0, span=1)[mode])
    tp = TourPlanner(_t(torch, data), goals, 2, mode=mode)
    paths, lens, stop_at = tp.plan(_t(torch, starts, torch.int32))
    assert (tp.status == 0).all() and np.array_equal(tp.fields.cpu().numpy(), want["fields"])
    assert np.array_equal(tp.start_cost.cpu().numpy(), want["start_cost"])
    assert np.array_equal(tp.task_cost.cpu().numpy(), want["task_cost"])
    out = want["out"]
    got = dict(tours=tp.tours, len=tp.tour_len, cost=tp.tour_cost, owner=tp.owner, count=tp.count, total=tp.total,
               span=tp.span, build_steps=tp.build_steps, rounds=tp.rounds)
    same({k: v.cpu().numpy() for k, v in got.items()}, out)
    assert out["count"] == 24 and ((out["len"] >= 1).all() or mode == "sum")   # (the least sum may leave a robot idle)
    P, L, SA = paths.cpu().numpy(), lens.cpu().numpy(), stop_at.cpu().numpy()
    assert np.array_equal(L, want["lens"]) and np.array_equal(SA, want["stop_at"])
    for b in range(16):
        route = P[b, :L[b]]
        n = out["len"][b]
        if n == 0:
            assert L[b] == 0 and (SA[b] == -1).all()
            continue
        assert route.tolist() == want["paths"][b, :L[b]].tolist() and route[0] == starts[b]
        dr, dc = np.abs(np.diff(route // S.W)), np.abs(np.diff(route % S.W))
        assert (np.maximum(dr, dc) == 1).all() and (data.ravel()[route] < 0.8).all()
        assert route[SA[b, :n]].tolist() == goals[out["tours"][b, :n]].tolist() and (SA[b, n:] == -1).all()
        assert SA[b, n - 1] == L[b] - 1
    assert np.array_equal(tp.goal_cells_of().cpu().numpy(), np.where(out["tours"] >= 0, goals[np.maximum(out["tours"], 0)], -1))
    # assign alone gives the same tours; the follower takes the plan as it is
    t2, l2 = tp.assign(_t(torch, starts, torch.int32))
    assert np.array_equal(t2.cpu().numpy(), out["tours"]) and np.array_equal(l2.cpu().numpy(), out["len"])
    fol = TourFollower(paths, lens, stop_at, S.W, S.x0, S.y0, S.cell)
    assert fol.served.shape == (16, 2) and int(fol.served_count().item()) == 0


# ---- refusals through ctypes, with device pointers ----------------------------------------------------------------------
def test_refusals_with_real_buffers_leave_them_untouched(rt):
    torch, lib = rt["torch"], rt["lib"]
    s, d = torch.ones((4, 6), dtype=torch.float64, device=DEV), torch.ones((6, 6), dtype=torch.float64, device=DEV)
    tours = torch.full((4, 2), -9, dtype=torch.int32, device=DEV)
    lens, cost = torch.full((4,), -9, dtype=torch.int32, device=DEV), torch.full((4,), -9, dtype=torch.int64, device=DEV)
    small = torch.zeros(lib.tours_work_bytes(1, 4, 6) - 1, dtype=torch.uint8, device=DEV)
    for kw, msg in ((dict(work=small), "the workspace holds"), (dict(scale=0.0), "scale"), (dict(max_rounds=-1), "max_rounds")):
        with pytest.raises(lib.RmpcError, match=msg):
            lib.tours_device(s, d, tours, lens, cost, **kw)
    with pytest.raises(lib.RmpcError, match="1 <= K <= T"):
        lib.tours_device(s, d, torch.zeros((4, 7), dtype=torch.int32, device=DEV), lens, cost)
    torch.cuda.synchronize()
    assert (tours == -9).all() and (lens == -9).all() and (cost == -9).all()
    with pytest.raises(lib.RmpcError, match="stop_tol"):
        lib.follow_tour_device(tours, lens, lens, s, s, 41, 0.0, 0.0, 0.5, 1.3, tours, lens, tours, 0, -1.0)


# ---- one closed loop ---------------------------------------------------------------------------------------------------
def test_sixteen_boxers_serve_twenty_four_picks(rt):
    """examples/fleet_store_tours.py, 16 boxers, 24 picks, K = 2, tours-span, seed 0, at most 400 control steps (the
    example's default, within which the dispatch run's 44-cell route arrives at step 92), leaving the loop once all picks
    are served: every pick is planned and served, and at most 1 % of the robot-steps fail (the gate of the timed-routes
    test)"""
    from example_loader import load_example
    ex = load_example("fleet_store_tours")
    r = ex.run(B=16, T=24, K=2, steps=400, seed=0, plan="tours-span")
    print(r)
    assert r["fused"] and r["picks_planned"] == 24 and r["picks_served"] == 24, r
    assert r["failed_share"] <= 0.01 and r["last_service_step"] <= r["steps"] <= 400, r
    with pytest.raises(ValueError):
        ex.run(B=4, T=9, K=2, steps=1)
