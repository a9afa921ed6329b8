"""Timed tours (include/rmpc_timed_tours.h), what needs no GPU: the two restatements of
tests/timed_tours_reference.py on hand-worked cases and against each other, the degenerate case against the timed
plan's restatement, the rule's properties, the follower's restatement, the store case the GPU closed loop rests on,
the fifth header and its tables, and every refusal of the three entries."""
import ctypes as C
import math

import numpy as np
import pytest

import timed_reference as timed
from timed_reference import OUTSIDE, conflicts, fields_for
from timed_support import I_MAX, NULL, P_, check_header, filled, load_lib, refused
from timed_tours_reference import INT32_MAX, follow_ref, plan_ref, plan_walk, store_tours_case

SYMBOLS = ["rmpc_timed_tours_work_bytes", "rmpc_timed_tours_plan_device", "rmpc_timed_tours_follow_device"]
BOTH = (plan_ref, plan_walk)
OUT = ("paths", "status", "arrive", "serve_at", "served", "unserved", "key", "best")
STORE_SEED = 0      # the first seed whose best of 16 orders has no failure and nothing unserved (test_store_case)


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def one(fn, grid, starts, cells, stops, lens, park, T, sep2=1, lag=1, dwell=0, orders=None, movement=4):
    """the plan of one order (the identity unless given) on the fields of ``cells``"""
    grid = np.asarray(grid, dtype=float)
    out = fn(grid, starts, stops, lens, park, fields_for(grid, cells, movement), cells,
             [np.arange(len(starts))] if orders is None else orders, T, sep2, lag, dwell, movement)
    return out


# ---- cases worked by hand ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", BOTH)
def test_corridor_two_stops_dwell_two(fn):
    out = one(fn, np.zeros((1, 7)), [0], [3, 6], [[0, 1]], [2], [1], 12, dwell=2)
    assert out["paths"][0, 0].tolist() == [0, 1, 2, 3, 3, 3, 4, 5, 6, 6, 6, 6, 6]
    assert out["serve_at"][0, 0].tolist() == [3, 8] and out["served"][0, 0] == 2 and out["unserved"][0] == 0
    assert out["status"][0, 0] == 0 and out["arrive"][0, 0] == 10          # the least a >= t0 = 8 + 2
    assert out["key"][0] == 10 and out["best"][0] == 0
    # the same tour with a return leg: park by the field of a third cell, the start
    out = one(fn, np.zeros((1, 7)), [0], [3, 6, 0], [[0, 1]], [2], [2], 18, dwell=2)
    assert out["paths"][0, 0].tolist() == [0, 1, 2, 3, 3, 3, 4, 5, 6, 6, 6, 5, 4, 3, 2, 1, 0, 0, 0]
    assert out["arrive"][0, 0] == 16


@pytest.mark.parametrize("fn", BOTH)
def test_the_start_on_the_first_stop(fn):
    out = one(fn, np.zeros((1, 7)), [3], [3, 6], [[0, 1]], [2], [1], 9, dwell=2)
    assert out["serve_at"][0, 0].tolist() == [0, 5]
    assert out["paths"][0, 0].tolist() == [3, 3, 3, 4, 5, 6, 6, 6, 6, 6] and out["arrive"][0, 0] == 7


@pytest.mark.parametrize("fn", BOTH)
def test_two_consecutive_stops_on_one_cell(fn):
    out = one(fn, np.zeros((1, 7)), [0], [3], [[0, 0]], [2], [0], 8, dwell=0)
    assert out["serve_at"][0, 0].tolist() == [3, 3] and out["paths"][0, 0].tolist() == [0, 1, 2, 3, 3, 3, 3, 3, 3]
    assert out["arrive"][0, 0] == 3
    out = one(fn, np.zeros((1, 7)), [0], [3], [[0, 0]], [2], [0], 8, dwell=1)
    assert out["serve_at"][0, 0].tolist() == [3, 4] and out["paths"][0, 0].tolist() == [0, 1, 2, 3, 3, 3, 3, 3, 3]
    assert out["arrive"][0, 0] == 5


@pytest.mark.parametrize("fn", BOTH)
def test_a_stop_behind_a_wall(fn):
    g = np.zeros((1, 7))
    g[0, 4] = 1.0
    out = one(fn, g, [1], [2, 6, 0], [[0, 1, 2]], [3], [2], 8)
    # stop 0 is served at 1; the field of cell 6 is +inf on this side of the wall, so the end cell is the least cell of
    # reach[T], cell 0, and the wait-first backtrack holds it as early as it can; stop 2 is never tried
    assert out["serve_at"][0, 0].tolist() == [1, -1, -1] and out["served"][0, 0] == 1 and out["unserved"][0] == 2
    assert out["status"][0, 0] == 0 and out["arrive"][0, 0] == 9
    assert out["paths"][0, 0].tolist() == [1, 2, 1, 0, 0, 0, 0, 0, 0]
    assert out["key"][0] == (1 << 32) | 9


@pytest.mark.parametrize("fn", BOTH)
def test_a_stop_a_higher_rank_parks_on(fn):
    out = one(fn, np.zeros((1, 7)), [3, 0], [3], [[0], [0]], [0, 1], [0, 0], 8)
    assert out["paths"][0, 0].tolist() == [3] * 9 and out["arrive"][0, 0] == 0
    assert out["serve_at"][0, 1].tolist() == [-1] and out["unserved"][0] == 1
    assert out["status"][0, 1] == 0 and out["arrive"][0, 1] == 9
    assert out["paths"][0, 1].tolist() == [0, 1, 2, 2, 2, 2, 2, 2, 2]       # as near as res lets it: D = 1 at cell 2
    # the other order serves it: the robot with the stop goes first, the parked one is exempt on its start
    two = one(fn, np.zeros((1, 7)), [3, 0], [3], [[0], [0]], [0, 1], [0, 0], 8, orders=[[0, 1], [1, 0]])
    assert two["unserved"].tolist() == [1, 0] and two["best"][0] == 1
    assert two["serve_at"][1, 1].tolist() == [3] and two["paths"][1, 1].tolist() == [0, 1, 2] + [3] * 6
    assert two["paths"][1, 0].tolist() == [3] + [4] * 8 and two["arrive"][1].tolist() == [9, 3]      # ... and makes way


@pytest.mark.parametrize("fn", BOTH)
def test_a_dwell_that_does_not_fit_the_window(fn):
    out = one(fn, np.zeros((1, 7)), [0], [6], [[0]], [1], [0], 7, dwell=2)
    assert out["serve_at"][0, 0].tolist() == [-1] and out["unserved"][0] == 1
    assert out["paths"][0, 0].tolist() == [0, 1, 2, 3, 4, 5, 6, 6] and out["status"][0, 0] == 0 and out["arrive"][0, 0] == 8
    out = one(fn, np.zeros((1, 7)), [0], [6], [[0]], [1], [0], 8, dwell=2)
    assert out["serve_at"][0, 0].tolist() == [6] and out["arrive"][0, 0] == 8


@pytest.mark.parametrize("fn", BOTH)
def test_a_held_test_that_fails_first_and_passes_later(fn):
    """5 x 5, robot 0 walks down column 2 (cells 2, 7, 12, 17, 22 at t = 0 .. 4) and stamps cell 12 into res[1 .. 3].
    Robot 1 stands on its stop, cell 12, with dwell 2: reach[0] holds 12 (the start is exempt), held fails on res[1];
    it steps aside, and 12 is in reach again at t = 4, where res[5], res[6] are clear."""
    out = one(fn, np.zeros((5, 5)), [2, 12], [22, 12], [[0], [1]], [0, 1], [0, 1], 10, dwell=2)
    assert out["paths"][0, 0, :6].tolist() == [2, 7, 12, 17, 22, 22]
    p = out["paths"][0, 1].tolist()
    assert out["serve_at"][0, 1].tolist() == [4] and p[0] == 12 and p[4:] == [12] * 7 and 12 not in p[1:4]
    assert out["status"][0].tolist() == [0, 0] and out["arrive"][0].tolist() == [4, 6]
    assert conflicts(out["paths"][0], out["status"][0], 5, 1, 1) == []


@pytest.mark.parametrize("fn", BOTH)
def test_swap_corridor_with_a_stop_in_the_bay(fn):
    """the corridor of DESIGN.md 18: row 1 of a 3 x 7 map and a bay above column 5.  Robot 1 yields into the bay, which
    is its stop with dwell 1, and goes on behind robot 0."""
    g = np.ones((3, 7))
    g[1, :] = 0.0
    g[0, 5] = 0.0
    out = one(fn, g, [7, 13], [13, 7, 5], [[0], [2]], [0, 1], [0, 1], 14, dwell=1)
    assert out["paths"][0, 0].tolist() == [7, 8, 9, 10, 11, 12] + [13] * 9
    assert out["paths"][0, 1].tolist() == [13, 12, 5, 5, 5, 5, 5, 12, 11, 10, 9, 8, 7, 7, 7]
    assert out["serve_at"][0, 1].tolist() == [2] and out["arrive"][0].tolist() == [6, 12] and out["unserved"][0] == 0
    assert conflicts(out["paths"][0], out["status"][0], 7, 1, 1) == []


@pytest.mark.parametrize("fn", BOTH)
def test_a_leg_that_fails_on_an_empty_layer(fn):
    """1 x 3: robot 0 walks from cell 2 to cell 0, where robot 1 stands (the later-ranked start is avoided during the
    first `lag` layers only).  res[1] then holds all three cells: robot 1's leg to its stop has an empty layer 1."""
    out = one(fn, np.zeros((1, 3)), [2, 0], [0, 2], [[0], [1]], [0, 1], [0, 1], 5)
    assert out["paths"][0].tolist() == [[2, 1, 0, 0, 0, 0], [0] * 6]
    assert out["status"][0].tolist() == [0, 1] and out["arrive"][0].tolist() == [2, 6]
    assert out["serve_at"][0, 1].tolist() == [-1] and out["unserved"][0] == 1
    assert out["key"][0] == (1 << 44) | (1 << 32) | 8


@pytest.mark.parametrize("fn", BOTH)
def test_skipped_robots_of_each_kind(fn):
    g = np.zeros((4, 4))
    cells = [5, 10]
    starts = [0, -1, 3, 12, 15, 16]
    stops = [[0, 1], [0, 1], [0, 2], [0, 1], [1, -1], [0, 1]]
    lens = [2, 1, 2, 3, 2, -1]
    park = [1, 1, 1, 1, 0, 2]
    out = one(fn, g, starts, cells, stops, lens, park, 9)
    # robot 0 is planned; 1: start outside; 2: a stop past Gf; 3: len > K; 4: a negative stop; 5: start past the map,
    # len < 0 and park past Gf
    assert out["status"][0].tolist() == [0] + [OUTSIDE] * 5
    assert (out["paths"][0, 1:] == -1).all() and (out["serve_at"][0, 1:] == -1).all() and (out["served"][0, 1:] == 0).all()
    assert out["arrive"][0].tolist() == [4] + [10] * 5
    assert out["unserved"][0] == 1 + 2 + 0 + 2 + 0               # a len out of range counts 0
    assert out["key"][0] == (5 << 32) | 54


# ---- the two restatements against each other --------------------------------------------------------------------------
def random_problem(seed):
    rng = np.random.default_rng(seed)
    H, W = (int(v) for v in rng.integers(1, 13, 2))
    if H * W < 6:
        H, W = 3, 4
    B, K = int(rng.integers(1, 6)), int(rng.integers(1, 4))
    g = (rng.uniform(size=(H, W)) < rng.choice([0.0, 0.15, 0.3])).astype(float)
    free = np.flatnonzero(g.ravel() < 0.5)
    if len(free) < B:
        g[:] = 0.0
        free = np.arange(H * W)
    starts = rng.choice(free, B, replace=False).astype(np.int32)
    Gf = int(rng.integers(1, 7))
    cells = rng.integers(0, H * W, Gf).astype(np.int32)          # (an occupied one now and then: never reached)
    stops = rng.integers(0, Gf, (B, K)).astype(np.int32)
    lens = rng.integers(0, K + 1, B).astype(np.int32)
    park = rng.integers(0, Gf, B).astype(np.int32)
    if seed % 9 == 0:                                             # a skipped robot
        kind, b = int(rng.integers(0, 4)), int(rng.integers(0, B))
        if kind == 0:
            starts[b] = H * W
        elif kind == 1:
            lens[b] = K + 1
        elif kind == 2:
            stops[b, 0], lens[b] = Gf, max(1, lens[b])
        else:
            park[b] = -1
    G = int(rng.integers(1, 4))
    orders = np.stack([rng.permutation(B) for _ in range(G)])
    if seed % 14 == 0:
        orders[-1, 0] = orders[-1, -1] if B > 1 else 1
    return dict(grid=g, start=starts, stops=stops, lens=lens, park_index=park, goal_cells=cells, orders=orders,
                T=int(rng.integers(1, 17)), sep2=int(rng.choice([1, 2, 4, 5])), lag=int(rng.integers(1, 3)),
                dwell=int(rng.integers(0, 4)), movement=int(rng.choice([4, 8])))


@pytest.fixture(scope="module")
def random_plans():
    plans = []
    for seed in range(200):
        q = random_problem(seed)
        q["fields"] = fields_for(q["grid"], q["goal_cells"], q["movement"])
        plans.append((q, plan_ref(**q)))
    return plans


def test_restatements_agree_on_random_problems(random_plans):
    seen = dict(unserved=0, failed=0, served=0, moves8=0)
    for q, a in random_plans:
        b = plan_walk(**q)
        for k in OUT:
            assert np.array_equal(a[k], b[k]), (k, q, a[k], b[k])
        ok = a["key"] < timed.INT64_MAX
        seen["unserved"] += int((a["unserved"][ok] > 0).sum())
        seen["failed"] += int((a["status"] > 0).sum())
        seen["served"] += int(a["served"].sum())
        seen["moves8"] += q["movement"] == 8
    assert all(v > 20 for v in seen.values()), seen


def test_properties_of_the_rule(random_plans):
    for q, out in random_plans:
        H, W = q["grid"].shape
        T, K, dwell, lag = q["T"], q["stops"].shape[1], q["dwell"], q["lag"]
        moves = [(0, 0)] + [(dc, dr) for dc, dr, _ in timed.MOVES[q["movement"]]]
        ranks = []
        for g in range(len(q["orders"])):
            if out["key"][g] == timed.INT64_MAX:
                assert (out["status"][g] == timed.BAD_ORDER).all() and out["unserved"][g] == INT32_MAX
                assert (out["serve_at"][g] == -1).all() and (out["served"][g] == 0).all() and (out["paths"][g] == -1).all()
                continue
            ranks.append((int(out["unserved"][g]), int(out["key"][g]), g))
            # the guarantee (the starts are drawn without regard to sep2: layer 0 against layer 0 is the caller's)
            assert [c for c in conflicts(out["paths"][g], out["status"][g], W, q["sep2"], lag) if c[2:] != (0, 0)] == []
            miss = 0
            for b in range(len(q["start"])):
                sa, p, n = out["serve_at"][g, b], out["paths"][g, b], int(q["lens"][b])
                if out["status"][g, b] == OUTSIDE:
                    miss += n if 0 <= n <= K else 0
                    continue
                m = int(out["served"][g, b])
                assert (sa[:m] >= 0).all() and (sa[m:] == -1).all() and m <= n
                assert (np.diff(sa[:m]) >= dwell).all()
                for j in range(m):
                    s = int(q["goal_cells"][q["stops"][b, j]])
                    assert sa[j] + dwell <= T and (p[sa[j]:sa[j] + dwell + 1] == s).all()
                miss += int((sa[:n] == -1).sum())
                assert p[0] == q["start"][b]
                for t in range(1, T + 1):                  # a wait or a legal move
                    assert ((p[t] % W - p[t - 1] % W), (p[t] // W - p[t - 1] // W)) in moves
                if m < n:
                    assert out["arrive"][g, b] == T + 1
            assert out["unserved"][g] == miss
        assert out["best"][0] == (min(ranks)[2] if ranks else -1)


def test_without_stops_it_is_the_timed_plan():
    hit = 0
    for seed in range(60):
        q = random_problem(seed)
        B = len(q["start"])
        fields = fields_for(q["grid"], q["goal_cells"], q["movement"])
        gi = q["park_index"].copy()
        if seed % 9 == 0:
            gi[0] = -1                                 # (the timed plan knows two kinds of skipped robot)
        for fn in BOTH:
            a = fn(q["grid"], q["start"], q["stops"], np.zeros(B, np.int32), gi, fields, q["goal_cells"], q["orders"],
                   q["T"], q["sep2"], q["lag"], q["dwell"], q["movement"])
            b = timed.plan_ref(q["grid"], q["start"], gi, fields, q["goal_cells"], q["orders"], q["T"], q["sep2"], q["lag"],
                               q["movement"])
            for k in ("paths", "status", "arrive", "key", "best"):
                assert np.array_equal(a[k], b[k]), (seed, k)
            assert (a["serve_at"] == -1).all() and (a["served"] == 0).all()
            assert all(u == (0 if key < timed.INT64_MAX else INT32_MAX) for u, key in zip(a["unserved"], a["key"]))
        hit += int((b["arrive"] <= q["T"]).sum())
    assert hit > 50


def test_best_ranks_unserved_before_the_key():
    """order 0 serves nothing but is early (robot 0 parks on robot 1's stop at once), order 1 serves the stop and has a
    failed robot: the greater key with nothing unserved wins"""
    out = one(plan_ref, np.zeros((1, 7)), [3, 0], [3], [[0], [0]], [0, 1], [0, 0], 8, orders=[[0, 1], [1, 0], [0, 0]])
    assert out["unserved"].tolist() == [1, 0, INT32_MAX] and out["key"][1] > out["key"][0] and out["best"][0] == 1


# ---- the follower -----------------------------------------------------------------------------------------------------
def test_follower_by_hand():
    # one robot on a 1 x 5 map, cell size 1: the plan 0 1 2 2 2 3 with stop 0 at layer 2 (dwell 2), stop 1 at layer 5
    paths = np.array([[0, 1, 2, 2, 2, 3]], np.int32)
    sa = np.array([[2, 5, -1]], np.int32)
    st = dict(idx=np.zeros(1, np.int32), leg=np.zeros(1, np.int32), served=np.full((1, 3), -1, np.int32))
    goal = np.zeros((1, 3))

    def step(x, now):
        st["idx"], g, blk, st["leg"], st["served"] = follow_ref(paths, st["idx"], np.array([[x, 0.0]]), goal, 5, 0.0, 0.0,
                                                                1.0, 0.6, 1, 1, sa, st["leg"], st["served"], now, 0.1)
        return int(st["idx"][0]), float(g[0, 0]), int(st["leg"][0])
    assert step(0.0, 0) == (1, 1.0, 0)
    assert step(0.5, 1) == (2, 2.0, 0)            # within threshold of cell 1
    assert step(1.5, 2) == (2, 2.0, 0)            # within threshold of the stop but not within stop_tol: stays, unserved
    assert step(1.95, 3) == (3, 2.0, 1)           # served at now = 3, and the advance of the same call
    assert step(1.95, 4) == (4, 2.0, 1)           # one advance per call: dwell 2 costs two steps
    assert step(1.95, 5) == (5, 3.0, 1)
    assert step(2.5, 6) == (5, 3.0, 1)            # the last layer is a stop: pending
    assert step(3.05, 7) == (5, 3.0, 2)
    assert st["served"].tolist() == [[3, 7, -1]]
    # two stops at one layer: one serve per call, no advance while the second is pending
    paths = np.array([[0, 0, 1]], np.int32)
    sa = np.array([[0, 0]], np.int32)
    a = follow_ref(paths, [0], np.zeros((1, 2)), goal, 5, 0.0, 0.0, 1.0, 0.6, 1, 1, sa, [0], [[-1, -1]], 4, 0.1)
    assert (a[0].tolist(), a[3].tolist(), a[4].tolist()) == ([0], [1], [[4, -1]])
    a = follow_ref(paths, a[0], np.zeros((1, 2)), goal, 5, 0.0, 0.0, 1.0, 0.6, 1, 1, sa, a[3], a[4], 5, 0.1)
    assert (a[0].tolist(), a[3].tolist(), a[4].tolist()) == ([1], [2], [[4, 5]])
    # an invalid path keeps everything; a negative leg counts as 0
    a = follow_ref(np.array([[-1, -1], [0, 1]], np.int32), [7, 0], np.zeros((2, 2)), np.full((2, 3), 9.0), 5, 0.0, 0.0, 1.0,
                   0.6, 1, 1, np.array([[0], [0]], np.int32), [5, -3], [[-1], [-1]], 2, 0.1)
    assert a[0].tolist() == [7, 1] and a[1][0].tolist() == [9.0] * 3 and a[3].tolist() == [5, 1] and a[4].tolist() == [[-1], [2]]


def test_follower_without_stops_is_the_timed_follower(random_plans):
    rng = np.random.default_rng(3)
    n = 0
    for q, out in random_plans[:80]:
        g = int(out["best"][0])
        if g < 0:
            continue
        paths, W, T = out["paths"][g], q["grid"].shape[1], q["T"]
        B, K = paths.shape[0], q["stops"].shape[1]
        idx = rng.integers(-1, T + 2, B)
        c = paths[np.arange(B), np.clip(idx, 0, T)]
        pos = np.stack([c % W + rng.choice([0.0, 0.05, 0.4], B), c // W + 0.0], 1)
        goal = rng.uniform(size=(B, 3))
        want = timed.follow_ref(paths, idx, pos, goal, W, 0.0, 0.0, 1.0, 0.1, q["sep2"], q["lag"])
        leg, served = rng.integers(0, K + 1, B), rng.integers(-1, 5, (B, K))
        got = follow_ref(paths, idx, pos, goal, W, 0.0, 0.0, 1.0, 0.1, q["sep2"], q["lag"], np.full((B, K), -1), leg, served,
                         3, 0.02)
        for a, b in zip(got[:3], want):
            assert np.array_equal(a, b)
        assert np.array_equal(got[3], leg) and np.array_equal(got[4], served)
        n += 1
    assert n > 40


def test_kinematic_walk_serves_every_stop_after_its_dwell(random_plans):
    """every robot jumps onto the waypoint it is given: the follower serves every planned stop, in order, never before
    its layer, and ends on the last layer"""
    n = 0
    for q, out in random_plans[:60]:
        g = int(out["best"][0])
        if g < 0 or (out["status"][g] == OUTSIDE).any():
            continue
        paths, sa, W, T = out["paths"][g], out["serve_at"][g], q["grid"].shape[1], q["T"]
        B, K = sa.shape
        idx, leg, served = np.zeros(B, np.int32), np.zeros(B, np.int32), np.full((B, K), -1, np.int32)
        pos = np.stack([paths[:, 0] % W, paths[:, 0] // W], 1).astype(float)
        goal = np.zeros((B, 3))
        for now in range(2 * T + 2 * K + 2):
            idx, goal, blk, leg, served = follow_ref(paths, idx, pos, goal, W, 0.0, 0.0, 1.0, 0.3, q["sep2"], q["lag"], sa, leg,
                                                     served, now, 0.1)
            pos = goal[:, :2].copy()
        assert (idx == T).all()
        assert np.array_equal(served >= 0, sa >= 0) and np.array_equal(leg, (sa >= 0).sum(1))
        assert (served[sa >= 0] >= sa[sa >= 0]).all()
        n += 1
    assert n > 30


# ---- the store case ---------------------------------------------------------------------------------------------------
def test_store_case_best_order_serves_everything():
    """16 starts and 24 picks in the store (store seed 0, on ``clear_cells(raw, 2)``, picks pairwise at least sep2 = 9
    apart, starts 25: the end links reach 0.4 m ahead of the base cells), tours from tests/tours_reference.py, K = 2,
    T = 255, dwell 3, 16 orders: the best order has no failed robot and nothing unserved.  Seed 0 gives it.  The GPU
    closed loop rests on this."""
    from robot_mpcs_amd.global_planner import priority_orders
    from robot_mpcs_amd.store import STORE
    import tours_reference
    raw, g_inf, starts, picks = store_tours_case(16, 24, STORE_SEED, 9)
    W = STORE.W
    assert len(starts) == 16 and len(picks) == 24
    assert all(timed._d2(int(a), int(b), W) >= 9 for i, a in enumerate(picks) for b in picks[:i])
    plan = tours_reference.plan_ref(g_inf, starts, picks, 2)
    tours, lens = plan["out"]["tours"], plan["out"]["len"]
    assert int(lens.sum()) == 24
    cells = np.concatenate([picks, starts]).astype(np.int32)
    fields = np.concatenate([plan["fields"], fields_for(g_inf, starts, 8)])
    park = np.where(lens > 0, tours[np.arange(16), np.maximum(lens, 1) - 1], 24 + np.arange(16)).astype(np.int32)
    orders = priority_orders(16, 16, 0)
    out = plan_ref(g_inf, starts, tours, lens, park, fields, cells, orders, 255, 9, 1, 3, 8)
    b = int(out["best"][0])
    print("store seed", STORE_SEED, "best", b, "unserved", out["unserved"].tolist(), "keys", out["key"].tolist())
    assert out["unserved"][b] == 0 and (out["status"][b] == 0).all()
    assert conflicts(out["paths"][b], out["status"][b], W, 9, 1) == []
    assert (out["arrive"][b] <= 255).all()


# ---- the header and the binding ---------------------------------------------------------------------------------------
def test_symbols_are_declared_by_the_new_header_and_exported(lib):
    from robot_mpcs_amd import _abi
    assert lib.TIMED_TOURS_SYMBOLS == SYMBOLS == list(_abi.timed_tours_prototypes)
    check_header(lib, "rmpc_timed_tours", SYMBOLS, _abi.timed_tours_prototypes)
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    S = _abi.timed_tours_structs["rmpc_timed_tours"]
    assert _abi.timed_tours_prototypes[SYMBOLS[0]] == (C.c_int64, [i] * 4)
    assert _abi.timed_tours_prototypes[SYMBOLS[1]] == (i, [C.POINTER(S), vp])
    assert _abi.timed_tours_prototypes[SYMBOLS[2]] == (i, [i, i, vp, vp, vp, vp, i, i, d, d, d, d, i, i, vp, vp, i, vp, vp, vp,
                                                           i, d, vp])
    assert _abi.timed_tours_constants == {"RMPC_TIMED_TOURS_MAX_STOPS": 64, "RMPC_TIMED_TOURS_MAX_DWELL": 64}
    assert (lib.TIMED_TOURS_MAX_STOPS, lib.TIMED_TOURS_MAX_DWELL) == (64, 64)
    # the struct: the timed plan's fields with goal_index replaced, then the added outputs
    mine, theirs = [f[0] for f in S._fields_], [f[0] for f in _abi.structs["rmpc_timed_plan"]._fields_]
    at = theirs.index("goal_index")
    assert mine == theirs[:at] + ["K", "dwell", "stops", "len", "park_index"] + theirs[at + 1:] + ["serve_at", "served", "unserved"]
    assert list(_abi.timed_tours_structs) == ["rmpc_timed_tours"] and C.sizeof(S) == 200
    # the other headers declare what they declared
    assert len(lib.EXPORTED_SYMBOLS) == 65 and len(lib.TOURS_SYMBOLS) == 3
    assert not set(SYMBOLS) & (set(_abi.prototypes) | set(_abi.tours_prototypes))


def test_work_bytes_is_the_timed_plans(lib):
    L = lib.load_library()
    for a in ((7, 5, 9, 2), (65, 70, 70, 3), (128, 128, 1023, 1024), (1, 1, 1, 1)):
        assert lib.timed_tours_work_bytes(*a) == lib.timed_plan_work_bytes(*a)
    for a in ((0, 5, 9, 2), (129, 128, 9, 1), (7, 5, 0, 2), (7, 5, 1024, 2), (7, 5, 9, 0), (7, 5, 9, 1025)):
        assert L.rmpc_timed_tours_work_bytes(*a) == -1 and L.rmpc_last_error().decode().startswith("timed tours")
        with pytest.raises(lib.RmpcError, match="timed tours"):
            lib.timed_tours_work_bytes(*a)


PLAN = dict(H=7, W=5, movement=4, grid=P_, occ_threshold=0.8, B=3, Gf=2, start_cell=P_, K=2, dwell=1, stops=P_, len=P_,
            park_index=P_, fields=P_, goal_cells=P_, T=9, sep2=2, lag=1, G=2, orders=P_, work=P_, work_bytes=1 << 20, paths=P_,
            status=P_, arrive=P_, key=P_, best=P_, serve_at=P_, served=P_, unserved=P_)
PLAN_REFUSALS = [(dict([(k, None)]), NULL) for k, v in PLAN.items() if v == P_]
PLAN_REFUSALS += [(dict(K=k), "timed tours: need 1 <= K <= RMPC_TIMED_TOURS_MAX_STOPS = 64") for k in (0, 65, -1, I_MAX)]
PLAN_REFUSALS += [(dict(dwell=v), "timed tours: need 0 <= dwell <= RMPC_TIMED_TOURS_MAX_DWELL = 64") for v in (-1, 65, I_MAX)]
PLAN_REFUSALS += [(dict(B=0), "timed tours: need 1 <= B"), (dict(B=1025), "timed tours: need 1 <= B"),
                  (dict(T=0), "timed tours: need 1 <= T"), (dict(T=1024), "timed tours: need 1 <= T"),
                  (dict(sep2=0), "timed tours: need 1 <= sep2"), (dict(sep2=4097), "timed tours: need 1 <= sep2"),
                  (dict(lag=0), "timed tours: lag must lie"), (dict(lag=5), "timed tours: lag must lie"),
                  (dict(G=0), "timed tours: need 1 <= G"), (dict(G=1025), "timed tours: need 1 <= G"),
                  (dict(movement=6), ""), (dict(H=0), ""), (dict(W=0), ""), (dict(H=129, W=128), ""), (dict(Gf=0), ""),
                  (dict(Gf=I_MAX), ""),
                  (dict(work_bytes=0), "timed tours: the workspace holds 0 bytes"),
                  (dict(work_bytes=-1), "timed tours: the workspace holds -1 bytes"),
                  (dict(struct_size=199), "rmpc_timed_tours.struct_size mismatch"),
                  (dict(struct_size=0), "rmpc_timed_tours.struct_size mismatch")]
# (G B (T + 1) and G B K beyond INT_MAX cannot be reached within the limits, 2^30 and 2^26 at the most; the entry checks
# both all the same, as the timed plan does)


@pytest.mark.parametrize("bad,want", PLAN_REFUSALS, ids=[",".join("%s=%s" % kv for kv in b.items()) for b, _ in PLAN_REFUSALS])
def test_plan_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    L = lib.load_library()
    assert set(bad) <= set(PLAN) | {"struct_size"}
    a = filled(lib.TimedToursArgs, PLAN, **bad)
    refused(L, L.rmpc_timed_tours_plan_device(C.byref(a), None), want)
    assert L.rmpc_timed_tours_plan_device(None, None) == -1 and L.rmpc_last_error().decode() == NULL


FOLLOW = dict(B=2, T=5, paths=P_, idx_in=P_, idx_out=P_ + 64, pos=P_, stride=3, W=41, x0=0.0, y0=0.0, cell=0.5, threshold=1.3,
              sep2=9, lag=1, goal=P_, blocked=None, K=2, serve_at=P_, leg=P_, served=P_, now=0, stop_tol=0.2, stream=None)
FOLLOW_REFUSALS = [(dict([(k, None)]), NULL) for k in ("paths", "idx_in", "idx_out", "pos", "goal", "serve_at", "leg", "served")]
FOLLOW_REFUSALS += [(dict(idx_out=P_), "timed tours follow: d_idx_out must not be d_idx_in"),
                    (dict(B=0), "timed tours follow: need 1 <= B"), (dict(T=0), "timed tours follow: need 1 <= T"),
                    (dict(sep2=0), "timed tours follow: need 1 <= sep2"), (dict(lag=5), "timed tours follow: lag must lie"),
                    (dict(K=0), "timed tours follow: need 1 <= K <= RMPC_TIMED_TOURS_MAX_STOPS = 64"),
                    (dict(K=65), "timed tours follow: need 1 <= K <= RMPC_TIMED_TOURS_MAX_STOPS = 64"),
                    (dict(stride=1), "timed tours follow: need stride >= 2, W >= 1"),
                    (dict(W=0), "timed tours follow: need stride >= 2, W >= 1"),
                    (dict(B=1024, stride=I_MAX), "timed tours follow: need stride >= 2, W >= 1"),
                    (dict(stop_tol=-0.1), "timed tours follow: stop_tol must be >= 0"),
                    (dict(stop_tol=math.nan), "timed tours follow: stop_tol must be >= 0"),
                    (dict(stop_tol=-math.inf), "timed tours follow: stop_tol must be >= 0")]


@pytest.mark.parametrize("bad,want", FOLLOW_REFUSALS, ids=[",".join("%s=%s" % kv for kv in b.items()) for b, _ in FOLLOW_REFUSALS])
def test_follow_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    L = lib.load_library()
    assert set(bad) <= set(FOLLOW)
    assert L.rmpc_timed_tours_follow_device(*dict(FOLLOW, **bad).values()) == -1
    assert L.rmpc_last_error().decode().startswith(want)
