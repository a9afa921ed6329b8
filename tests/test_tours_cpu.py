"""Tours of several tasks per robot (include/rmpc_tours.h), what needs no GPU: the two restatements of
tests/tours_reference.py on hand-worked cases and against each other, the rule's properties, a brute force over all
partitions and orders, the follower that stops on a kinematic walk through the store, the fourth header and its tables,
and every refusal of the three entries."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tours_cases import KINDS, make_problem, small_integer_problem, store_draw
from tours_reference import (brute_force, follow_tour_loop, follow_tour_ref, objective, plan_ref, quantise, tour_cost,
                             tours_loop, tours_problem_ref, tours_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = math.inf, math.nan
SYMBOLS = ["rmpc_tours_work_bytes", "rmpc_tours_device", "rmpc_follow_tour_device"]
BOTH = (tours_ref, tours_loop)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return _lib


def line(starts, tasks):
    """costs of points on a line: |x - y|"""
    s, t = np.asarray(starts, dtype=np.int64), np.asarray(tasks, dtype=np.int64)
    return np.abs(s[:, None] - t[None, :]), np.abs(t[:, None] - t[None, :])


def tours_of(out):
    return [out["tours"][b, :out["len"][b]].tolist() for b in range(len(out["len"]))]


# ---- cases worked by hand ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", BOTH)
def test_two_robots_on_a_line(fn):
    """robots at 0 and 10, tasks at 1, 2, 8, 9.  mode 0: (delta 1: 0 -> t0), (1: 1 -> t3; b = 0 comes first on the tie),
    (1: t1 behind t0), (1: t2 in front of t3): tours [0, 1] and [3, 2], both of cost 2"""
    qs, qt = line([0, 10], [1, 2, 8, 9])
    for mode in (0, 1):
        out = fn(qs, qt, 2, mode, 10)
        assert tours_of(out) == [[0, 1], [3, 2]] and out["cost"].tolist() == [2, 2]
        assert (out["count"], out["total"], out["span"], out["build_steps"], out["rounds"]) == (4, 4, 2, 4, 0)
        assert out["owner"].tolist() == [0, 0, 1, 1]


@pytest.mark.parametrize("fn", BOTH)
def test_an_insertion_with_a_negative_delta(fn):
    """one robot, costs that are no metric.  t1 first (delta e(s, 1) = 1).  Then t0 in front of it,
    e(s, 0) + e(0, 1) - e(s, 1) = 2 + 10 - 1 = 11, against 50 for every other candidate: [0, 1] of cost 12.  Then t2
    between them, e(0, 2) + e(2, 1) - e(0, 1) = 1 + 1 - 10 = -8 (in front 50 + 50 - 2, behind 50): [0, 2, 1] of cost 4"""
    qs = np.array([[2, 1, 50]])
    qt = np.array([[0, 10, 1], [50, 0, 50], [50, 1, 0]])
    two = fn(qs[:, :2], qt[:2, :2], 3, 0, 0)
    assert tours_of(two) == [[0, 1]] and two["cost"].tolist() == [12]
    for mode in (0, 1):
        out = fn(qs, qt, 3, mode, 0)
        assert tours_of(out) == [[0, 2, 1]] and out["cost"].tolist() == [4] and out["build_steps"] == 3
        assert fn(qs, qt, 3, mode, 9)["rounds"] == 0                       # nothing to improve


@pytest.mark.parametrize("fn", BOTH)
def test_a_hole_forbids_a_bridge(fn):
    """one robot, tour [0, 1, 2] with e(0, 2) not takeable: t1 cannot be taken out, though moving it to the end would
    save; t2 in front of everything is what remains"""
    qs = np.array([[1, 50, 3]])
    qt = np.array([[0, 9, -1], [1, 0, 1], [1, 1, 0]])
    start = [[0, 1, 2]]
    assert tour_cost(qs, qt, 0, start[0]) == 11
    out = fn(qs, qt, 3, 0, 10, improve_from=start)
    # relocations of t1 are barred (the bridge 0 -> 2); t0 to the end: 50 + 1 + 1 = 52; t2 to the front: 3 + 1 + 9 = 13;
    # t2 between: 1 + -1: barred; exchanges: (0, 1): [1, 0, 2] barred (0 -> 2); (0, 2): [2, 1, 0] = 3 + 1 + 1 = 5; (1, 2):
    # [0, 2, 1] barred
    assert tours_of(out) == [[2, 1, 0]] and out["cost"].tolist() == [5] and out["rounds"] == 1
    qt[0, 2] = 0                                                           # the bridge opens: t1 leaves first
    out = fn(qs, qt, 3, 0, 1, improve_from=start)
    assert tours_of(out) == [[0, 2, 1]] and out["cost"].tolist() == [2]


@pytest.mark.parametrize("fn", BOTH)
def test_full_tours_leave_only_the_exchange(fn):
    """two robots with K = 1 holding each other's near task: no relocation has room, the exchange halves the cost"""
    qs, qt = line([0, 10], [9, 1])
    for mode in (0, 1):
        out = fn(qs, qt, 1, mode, 5, improve_from=[[0], [1]])
        assert tours_of(out) == [[1], [0]] and out["cost"].tolist() == [1, 1] and out["rounds"] == 1


@pytest.mark.parametrize("fn", BOTH)
def test_max_rounds_zero_and_the_cap(fn):
    s, d = make_problem("unif", 3, 9)
    qs, qt = quantise(s, 1.0), quantise(d, 1.0)
    free = fn(qs, qt, 4, 0, 1 << 30)
    assert free["rounds"] >= 2
    build = fn(qs, qt, 4, 0, 0)
    assert build["rounds"] == 0 and build["build_steps"] == 9 and build["total"] > free["total"]
    capped = fn(qs, qt, 4, 0, free["rounds"] - 1)
    assert capped["rounds"] == free["rounds"] - 1 and build["total"] > capped["total"] > free["total"]
    again = fn(qs, qt, 4, 0, free["rounds"])
    assert again["rounds"] == free["rounds"] and np.array_equal(again["tours"], free["tours"])


def test_mode_one_may_raise_the_sum_but_not_the_span():
    """robots at 0 and 100; after the build one tour is long; the improvement evens them out"""
    qs, qt = line([0, 3], [10, 20, 30, 40])
    for fn in BOTH:
        a, b = fn(qs, qt, 4, 1, 0), fn(qs, qt, 4, 1, 50)
        assert b["span"] <= a["span"]
        s0, s1 = fn(qs, qt, 4, 0, 0), fn(qs, qt, 4, 0, 50)
        assert s1["total"] <= s0["total"]


# ---- the two restatements against each other --------------------------------------------------------------------------
def same(a, b):
    for key in a:
        assert np.array_equal(a[key], b[key]), (key, a[key], b[key])


def test_restatements_agree_on_random_problems():
    rng = np.random.default_rng(24)
    moved = 0
    for trial in range(200):
        B, T = int(rng.integers(1, 5)), int(rng.integers(1, 10))
        K = int(rng.integers(1, T + 1))
        qs, qt = small_integer_problem(rng, B, T, holes=trial % 2 == 1)
        mode = trial // 2 % 2
        cap = [1 << 30, 1 << 30, 0, 2][trial % 4]
        a, b = tours_ref(qs, qt, K, mode, cap), tours_loop(qs, qt, K, mode, cap)
        same(a, b)
        moved += a["rounds"]
        check_properties(qs, qt, K, a)
    assert moved > 20                                                      # the improvement was at work


def test_restatements_agree_on_the_improvement_of_random_tours():
    """improvement from tours that no build made: random partitions in random order, holes between them"""
    rng = np.random.default_rng(25)
    for trial in range(60):
        B, T = int(rng.integers(1, 5)), int(rng.integers(2, 10))
        qs, qt = small_integer_problem(rng, B, T, holes=trial % 3 == 0)
        K = int(rng.integers(1, T + 1))
        tours = [[] for _ in range(B)]
        for t in rng.permutation(T):
            b = int(rng.integers(0, B))
            if len(tours[b]) < K and tour_cost(qs, qt, b, tours[b] + [int(t)]) is not None:
                tours[b].append(int(t))
        for mode in (0, 1):
            same(tours_ref(qs, qt, K, mode, 1 << 30, improve_from=tours), tours_loop(qs, qt, K, mode, 1 << 30, improve_from=tours))


# ---- properties -------------------------------------------------------------------------------------------------------
def check_properties(qs, qt, K, out):
    held = [t for tour in tours_of(out) for t in tour]
    assert len(held) == len(set(held)) == out["count"] and (out["len"] <= K).all()
    for b, tour in enumerate(tours_of(out)):
        assert tour_cost(qs, qt, b, tour) == out["cost"][b]
        assert (out["owner"][tour] == b).all() and (out["tours"][b, len(tour):] == -1).all()
    assert (out["owner"] >= 0).sum() == out["count"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,T,K", [(3, 20, 7), (5, 33, 7), (8, 12, 1), (2, 30, 30)])
def test_properties_of_the_rule(kind, B, T, K):
    s, d = make_problem(kind, B, T)
    qs, qt = quantise(s), quantise(d)
    for mode in (0, 1):
        built, out = tours_ref(qs, qt, K, mode, 0), tours_ref(qs, qt, K, mode, 1 << 30)
        for o in (built, out):
            check_properties(qs, qt, K, o)
            assert o["count"] == min(T, B * K) == o["build_steps"]       # every edge takeable: nothing is left over
        assert objective(out, mode) <= objective(built, mode)
        # round by round the sum (mode 0) / the span (mode 1) never rises
        trace = [objective(tours_ref(qs, qt, K, mode, r), mode) for r in range(min(out["rounds"], 12) + 1)]
        assert all(b <= a for a, b in zip(trace, trace[1:])), trace
        if mode == 0:
            assert all(b < a for a, b in zip(trace, trace[1:]))
    sh, dh = make_problem(kind, B, T, holes=True)
    for mode in (0, 1):
        check_properties(quantise(sh), quantise(dh), K, tours_ref(quantise(sh), quantise(dh), K, mode, 1 << 30))


def test_against_a_brute_force_over_all_partitions_and_orders():
    """the rule's objective is never below the optimum; how far above it is a measurement, printed here"""
    rng = np.random.default_rng(26)
    worst = {(mode, when): 1.0 for mode in (0, 1) for when in ("build", "improved")}
    for trial in range(40):
        B, T = int(rng.integers(1, 4)), int(rng.integers(2, 8))
        K = int(rng.integers(-(-T // B), T + 1))
        if trial % 2:
            qs, qt = small_integer_problem(rng, B, T, holes=False)
            qs, qt = qs + 1, qt + 1
        else:
            cells = rng.integers(0, 30, size=(B + T, 2))
            dist = np.rint(16 * np.hypot(*(cells[:, None, :] - cells[None, :, :]).transpose(2, 0, 1))).astype(np.int64)
            qs, qt = dist[:B, B:], dist[B:, B:]
        for mode in (0, 1):
            best = brute_force(qs, qt, K, mode)
            for when, cap in (("build", 0), ("improved", 1 << 30)):
                out = tours_ref(qs, qt, K, mode, cap)
                assert out["count"] == T and objective(out, mode) >= best
                worst[(mode, when)] = max(worst[(mode, when)], objective(out, mode) / best)
    print("worst ratio to the optimum:", {k: round(v, 3) for k, v in worst.items()})


# ---- the follower -----------------------------------------------------------------------------------------------------
def test_follower_restatements_agree_on_constructed_indices():
    rng = np.random.default_rng(27)
    B, K, L, W = 40, 3, 12, 41
    for trial in range(30):
        paths = rng.integers(0, W * W, size=(B, L)).astype(np.int32)
        lens = rng.integers(0, L + 1, size=B).astype(np.int32)
        stop_at = np.sort(rng.integers(0, L, size=(B, K)), axis=1).astype(np.int32)
        stop_at[rng.uniform(size=B) < 0.3, K - 1] = -1
        idx = rng.integers(0, L, size=B).astype(np.int32)
        idx[::2] = stop_at[::2, 0]
        leg = rng.integers(0, K + 1, size=B).astype(np.int32)
        leg[::2] = 0
        cells = paths[np.arange(B), np.clip(idx, 0, np.maximum(lens, 1) - 1)]
        pos = np.stack([-9.0 + (cells % W) * 0.45, -9.0 + (cells // W) * 0.45, np.zeros(B)], 1)
        pos[:, :2] += rng.choice([0.0, 0.1, 0.5, 2.0], size=(B, 1))
        state = [(idx.copy(), leg.copy(), np.full((B, K), -7, dtype=np.int32)) for _ in range(2)]
        g1 = follow_tour_ref(paths, lens, state[0][0], pos, W, -9.0, -9.0, 0.45, 1.3, stop_at, state[0][1], state[0][2], trial, 0.3)
        g2 = follow_tour_loop(paths, lens, state[1][0], pos, W, -9.0, -9.0, 0.45, 1.3, stop_at, state[1][1], state[1][2], trial, 0.3)
        assert np.array_equal(g1, g2, equal_nan=True)
        for x, y in zip(*state):
            assert np.array_equal(x, y)
        assert (state[0][2] != -7).any()


def test_follower_by_hand():
    """one robot on a straight path of 4 cells with stops at 1, 1 and 3: it waits at cell 1 until within stop_tol, serves
    both stops in two calls, moves on, and serves the last cell where it stays"""
    W, paths, lens = 10, np.array([[0, 1, 2, 3]], dtype=np.int32), np.array([4], dtype=np.int32)
    stop_at = np.array([[1, 1, 3]], dtype=np.int32)
    for fn in (follow_tour_ref, follow_tour_loop):
        idx, leg, served = np.zeros(1, np.int32), np.zeros(1, np.int32), np.full((1, 3), -1, np.int32)
        step = lambda x, now: fn(paths, lens, idx, np.array([[x, 0.0]]), W, 0.0, 0.0, 1.0, 1.3, stop_at, leg, served, now, 0.2)
        assert step(0.0, 0)[0].tolist() == [1.0, 0.0, 0.0] and idx[0] == 1          # cell 0 is no stop: on
        step(0.5, 1)
        assert (idx[0], leg[0]) == (1, 0)                                            # within 1.3 but not within 0.2: waits
        step(0.9, 2)
        assert (idx[0], leg[0], served.tolist()) == (1, 1, [[2, -1, -1]])            # served; the next stop is here too
        step(0.9, 3)
        assert (idx[0], leg[0], served.tolist()) == (2, 2, [[2, 3, -1]])
        step(1.0, 4)
        assert idx[0] == 3
        step(2.9, 5)
        assert (idx[0], leg[0], served.tolist()) == (3, 3, [[2, 3, 5]])
        assert step(2.9, 6)[0].tolist() == [3.0, 0.0, 0.0] and (idx[0], leg[0], served.tolist()) == (3, 3, [[2, 3, 5]])


@pytest.fixture(scope="module")
def store_plan():
    data, starts, goals = store_draw(16, 24, seed=0)
    return data, starts, goals, plan_ref(data, starts, goals, 2, mode=1)


def test_kinematic_walk_through_the_store_serves_every_pick(store_plan):
    """16 robots, 24 picks, K = 2, seed 0 on the store: points that move 0.2 m per step towards the follower's goal serve
    every pick, each robot's in ascending order of time"""
    from robot_mpcs_amd.store import STORE as S
    data, starts, goals, plan = store_plan
    out = plan["out"]
    assert out["count"] == 24 and (out["len"] <= 2).all()
    B, K = 16, 2
    pos = np.stack([S.x0 + (starts % S.W) * S.cell, S.y0 + (starts // S.W) * S.cell], 1).astype(np.float64)
    idx, leg, served = np.zeros(B, np.int32), np.zeros(B, np.int32), np.full((B, K), -1, np.int32)
    goal = np.concatenate([pos, np.zeros((B, 1))], 1)
    for now in range(600):
        new = follow_tour_ref(plan["paths"], plan["lens"], idx, pos, S.W, S.x0, S.y0, S.cell, 1.3, plan["stop_at"], leg,
                              served, now, 0.25)
        goal = np.where(np.isnan(new), goal, new)
        d = goal[:, :2] - pos
        n = np.linalg.norm(d, axis=1, keepdims=True)
        pos = pos + d * np.minimum(1.0, 0.2 / np.maximum(n, 1e-12))
        if (leg == out["len"]).all():
            break
    assert (leg == out["len"]).all() and (served >= 0).sum() == 24
    for b in range(B):
        s = served[b, :out["len"][b]]
        assert (s >= 0).all() and (np.diff(s) >= 0).all() and (served[b, out["len"][b]:] == -1).all()
        cells = plan["paths"][b, plan["stop_at"][b, :out["len"][b]]]
        assert cells.tolist() == goals[out["tours"][b, :out["len"][b]]].tolist()


# ---- the header and the binding ---------------------------------------------------------------------------------------
def test_tours_symbols_are_declared_by_the_new_header_and_exported(lib):
    from robot_mpcs_amd import _abi
    assert lib.TOURS_SYMBOLS == SYMBOLS == list(_abi.tours_prototypes)
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rmpc_tours.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(rmpc_\w+)\s*\(", code))) == sorted(SYMBOLS)
    L = lib.load_library()
    for sym in SYMBOLS:
        fn = getattr(L, sym)
        assert (fn.restype, list(fn.argtypes)) == (_abi.tours_prototypes[sym][0], _abi.tours_prototypes[sym][1])
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    assert _abi.tours_prototypes[SYMBOLS[0]] == (C.c_int64, [i] * 3)
    assert _abi.tours_prototypes[SYMBOLS[1]] == (i, [i] * 4 + [vp, vp, i, d, i] + [vp] * 10 + [C.c_int64, vp])
    assert _abi.tours_prototypes[SYMBOLS[2]] == (i, [i, vp, vp, i, vp, vp, i, i, d, d, d, d, vp, i, vp, vp, vp, i, d, vp])
    assert _abi.tours_constants == {"RMPC_TOURS_MAX_ROBOTS": 1024, "RMPC_TOURS_MAX_TASKS": 1024}
    assert (lib.TOURS_MAX_ROBOTS, lib.TOURS_MAX_TASKS) == (1024, 1024)
    # the three other headers declare what they declared
    assert len(lib.EXPORTED_SYMBOLS) == 65 and len(lib.GRID_LARGE_SYMBOLS) == 2 and len(lib.ASSIGN_OPT_SYMBOLS) == 2
    assert not set(SYMBOLS) & (set(_abi.prototypes) | set(_abi.large_prototypes) | set(_abi.assign_prototypes))
    with open(os.path.join(ROOT, "robot_mpcs_amd", "csrc", "sources.txt")) as f:
        listed = f.read().split()
    assert "include/rmpc_tours.h" in listed and "robot_mpcs_amd/csrc/rmpc_tours.hpp" in listed


I_MAX, I_MIN = 2 ** 31 - 1, -2 ** 31
SIZES = ": need 1 <= B <= RMPC_TOURS_MAX_ROBOTS = 1024 and 1 <= T <= RMPC_TOURS_MAX_TASKS = 1024"
G_TT = ": need 1 <= G, G*T*T <= INT_MAX and G*B*T <= INT_MAX"
BAD_SIZES = [(dict(B=0), SIZES), (dict(B=1025), SIZES), (dict(T=0), SIZES), (dict(T=1025), SIZES), (dict(B=I_MIN), SIZES),
             (dict(T=I_MAX), SIZES), (dict(G=0), G_TT), (dict(G=-1), G_TT), (dict(G=I_MIN), G_TT),
             (dict(G=2048, B=1, T=1024), G_TT), (dict(G=I_MAX, B=2, T=1), G_TT), (dict(G=0, B=0), SIZES)]


def test_work_bytes_is_host_only_and_refuses_bad_sizes(lib):
    L = lib.load_library()
    wb = lib.tours_work_bytes
    assert wb(1, 1, 1) == 20 and wb(3, 5, 7) == 4 * 3 * (105 + 98) and wb(1, 1024, 1024) == 20 << 20
    assert wb(2047, 1, 1024) == 4 * 2047 * (3 * 1024 + 2 * 1024 * 1024) and wb(I_MAX, 1, 1) == 20 * I_MAX
    for bad, want in BAD_SIZES:
        a = dict(dict(G=1, B=4, T=4), **bad)
        assert L.rmpc_tours_work_bytes(a["G"], a["B"], a["T"]) == -1
        assert L.rmpc_last_error().decode() == "tours work bytes" + want
        with pytest.raises(lib.RmpcError, match="tours work bytes"):
            wb(a["G"], a["B"], a["T"])


P_ = 0x1000      # a host-side fake pointer: a refusal never dereferences it
ARGS = dict(G=1, B=4, T=6, K=2, start=P_, task=P_, mode=1, scale=1024.0, max_rounds=5, tours=P_, len=P_, cost=P_,
            owner=None, count=None, total=None, span=None, build=None, rounds=None, work=P_, bytes=1 << 20, stream=None)
NULL = "null argument"
REFUSALS = [(dict([(k, None)]), NULL) for k in ("start", "task", "tours", "len", "cost", "work")]
REFUSALS += [(bad, "tours" + want) for bad, want in BAD_SIZES]
REFUSALS += [(dict(K=k), "tours: need 1 <= K <= T") for k in (0, 7, -1, I_MAX)]
REFUSALS += [(dict(mode=m), "tours: mode must be 0 (least sum) or 1 (least makespan)") for m in (2, -1)]
REFUSALS += [(dict(scale=s), "tours: scale must be finite and > 0") for s in (0.0, -1.0, NAN, INF, -INF)]
REFUSALS += [(dict(max_rounds=-1), "tours: max_rounds must be >= 0")]
NEED = 4 * (72 + 72)
REFUSALS += [(dict(bytes=b), "tours: the workspace holds %d bytes, %d are needed (rmpc_tours_work_bytes)" % (b, NEED))
             for b in (NEED - 1, 0, -5)]
REFUSALS += [(dict(start=None, B=0), NULL), (dict(B=0, K=0), "tours" + SIZES), (dict(K=0, bytes=0), "tours: need 1 <= K <= T")]


@pytest.mark.parametrize("bad,want", REFUSALS, ids=[",".join("%s=%s" % kv for kv in b.items()) for b, _ in REFUSALS])
def test_tours_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    L = lib.load_library()
    assert set(bad) <= set(ARGS)
    assert L.rmpc_tours_device(*dict(ARGS, **bad).values()) == -1
    assert L.rmpc_last_error().decode() == want


FOLLOW = dict(B=2, path=P_, len=P_, max_len=8, idx=P_, pos=P_, stride=3, W=41, x0=0.0, y0=0.0, cell=0.5, threshold=1.3,
              goal=P_, K=2, stop_at=P_, leg=P_, served=P_, now=0, stop_tol=0.2, stream=None)
B_LEN = "follow tour: need B, max_len >= 1 and B*max_len <= INT_MAX"
FOLLOW_REFUSALS = [(dict([(k, None)]), NULL) for k in ("path", "len", "idx", "pos", "goal", "stop_at", "leg", "served")]
FOLLOW_REFUSALS += [(dict(B=0), B_LEN), (dict(max_len=0), B_LEN), (dict(B=1 << 20, max_len=1 << 12), B_LEN),
                    (dict(K=0), "follow tour: need K >= 1 and B*K <= INT_MAX"),
                    (dict(B=1 << 16, K=1 << 16), "follow tour: need K >= 1 and B*K <= INT_MAX"),
                    (dict(stride=1), "follow tour: need stride >= 2, W >= 1"), (dict(W=0), "follow tour: need stride >= 2, W >= 1"),
                    (dict(stop_tol=-0.1), "follow tour: stop_tol must be >= 0"), (dict(stop_tol=NAN), "follow tour: stop_tol must be >= 0")]


@pytest.mark.parametrize("bad,want", FOLLOW_REFUSALS, ids=[",".join("%s=%s" % kv for kv in b.items()) for b, _ in FOLLOW_REFUSALS])
def test_follow_tour_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    L = lib.load_library()
    assert set(bad) <= set(FOLLOW)
    assert L.rmpc_follow_tour_device(*dict(FOLLOW, **bad).values()) == -1
    assert L.rmpc_last_error().decode() == want


def test_wrapper_refuses_mismatched_tensors(lib):
    import torch
    s, d = torch.zeros((2, 3, 4), dtype=torch.float64), torch.zeros((2, 4, 4), dtype=torch.float64)
    tours, lens, cost = torch.zeros((2, 3, 2), dtype=torch.int32), torch.zeros((2, 3), dtype=torch.int32), torch.zeros((2, 3), dtype=torch.int64)
    for args, kw in (((s.float(), d, tours, lens, cost), {}), ((s, d[0], tours, lens, cost), {}), ((s, d, tours, lens[0], cost), {}),
                     ((s, d, tours, lens, cost.int()), {}), ((s, d[:, :3], tours, lens, cost), {}),
                     ((s, d, tours, lens, cost), dict(mode="best")), ((s, d, tours, lens, cost), dict(owner=torch.zeros((2, 3), dtype=torch.int32))),
                     ((s, d, tours, lens, cost), dict(total=torch.zeros(2, dtype=torch.int32))),
                     ((s, d, tours, lens, cost), dict(rounds=torch.zeros(3, dtype=torch.int32)))):
        with pytest.raises(ValueError, match="tours_device"):
            lib.tours_device(*args, **kw)
