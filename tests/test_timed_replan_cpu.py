"""Lifelong timed tours (include/rmpc_timed_replan.h), what needs no GPU: the two restatements of
tests/timed_replan_reference.py on hand-worked cases and against each other, the identities C1 to C3 that tie the re-plan
to the timed tours' restatement, the guarantee (C4) with a pair checker of its own, clash (C5), ``rebase`` on torch CPU
tensors, the sixth header and its tables, and the refusals of the four entries."""
import ctypes as C

import numpy as np
import pytest

import timed_reference as timed
from timed_reference import BAD_ORDER, OUTSIDE, fields_for
from timed_replan_reference import KEPT, rebase_ref, replan_ref, replan_walk, reserve_ref, table_words
from timed_support import I_MAX, NULL, P_, check_header, filled, load_lib, refused
from timed_tours_reference import INT32_MAX, plan_ref

SYMBOLS = ["rmpc_timed_reserve_words", "rmpc_timed_reserve_device", "rmpc_timed_replan_work_bytes",
           "rmpc_timed_tours_replan_device"]
BOTH = (replan_ref, replan_walk)
OUT = ("paths", "status", "arrive", "serve_at", "served", "unserved", "key", "best")


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def one(fn, grid, starts, cells, stops, lens, park, T, sep2=1, lag=1, dwell=0, orders=None, movement=4, reserved=(), active=None,
        begin=None):
    """the re-plan of one order (the identity unless given) on the fields of ``cells``; ``reserved``: paths of sep2"""
    grid = np.asarray(grid, dtype=float)
    H, W = grid.shape
    table = dict(reserved_paths=[(q, sep2) for q in reserved]) if fn is replan_walk else dict(
        res0=reserve_ref(H, W, T, np.array(reserved), sep2, lag) if len(reserved) else None)
    return fn(grid, starts, stops, lens, park, fields_for(grid, cells, movement), cells,
              [np.arange(len(starts))] if orders is None else orders, T, sep2, lag, dwell, movement, active=active, begin=begin,
              **table)


# ---- cases worked by hand ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", BOTH)
def test_corridor_where_the_replanned_robot_waits_for_a_kept_one(fn):
    """1 x 7.  The kept robot stands on cell 3 up to layer 2 and walks to cell 6: its route holds cell 3 in res[0 .. 3] and
    cell 4 in res[2 .. 4].  The re-planned robot, from cell 0 to its stop on cell 4, waits one layer on cell 2; alone it
    is served at layer 4."""
    kept = [3, 3, 3, 4, 5, 6, 6, 6, 6, 6]
    out = one(fn, np.zeros((1, 7)), [0, 3], [4], [[0], [0]], [1, 0], [0, 0], 9, reserved=[kept], active=[1, 0])
    assert out["paths"][0, 0].tolist() == [0, 1, 2, 2, 3, 4, 4, 4, 4, 4] and out["serve_at"][0, 0].tolist() == [5]
    assert out["status"][0].tolist() == [0, KEPT] and out["arrive"][0].tolist() == [5, 0] and out["served"][0].tolist() == [1, 0]
    assert (out["paths"][0, 1] == -1).all() and out["unserved"][0] == 0 and out["key"][0] == 5 and out["clash"].tolist() == [0, 0]
    alone = one(fn, np.zeros((1, 7)), [0, 3], [4], [[0], [0]], [1, 0], [0, 0], 9, active=[1, 0])
    assert alone["serve_at"][0, 0].tolist() == [4]


@pytest.mark.parametrize("fn", BOTH)
@pytest.mark.parametrize("order", [[0, 1], [1, 0]])
def test_a_start_is_held_until_its_begin_layer_plus_lag(fn, order):
    """1 x 7.  Robot 0 stands on cell 3 until its begin layer 3 and then parks on cell 6; robot 1 has its stop on cell 3.
    Whatever the rank, cell 3 is barred to robot 1 while t <= 3 + lag: it is served at layer 5, never at layer 3, where
    the old rule (t <= lag) let it in before robot 0 is planned."""
    out = one(fn, np.zeros((1, 7)), [3, 0], [3, 6], [[0], [0]], [0, 1], [1, 0], 9, orders=[order], begin=[3, 0])
    assert out["paths"][0].tolist() == [[3, 3, 3, 3, 4, 5, 6, 6, 6, 6], [0, 1, 2, 2, 2, 3, 3, 3, 3, 3]]
    assert out["serve_at"][0, 1].tolist() == [5] and out["status"][0].tolist() == [0, 0] and out["arrive"][0].tolist() == [6, 5]
    old = one(fn, np.zeros((1, 7)), [3, 0], [3, 6], [[0], [0]], [0, 1], [1, 0], 9, orders=[[1, 0]])
    assert old["serve_at"][0, 1].tolist() == [3]


@pytest.mark.parametrize("fn", BOTH)
def test_a_kept_robot_in_a_bad_row(fn):
    out = one(fn, np.zeros((1, 7)), [0, 3], [4], [[0], [0]], [1, 0], [0, 0], 9, orders=[[0, 1], [1, 1]], active=[1, 0])
    assert out["status"].tolist() == [[0, KEPT], [BAD_ORDER, BAD_ORDER]] and out["arrive"][1].tolist() == [10, 10]
    assert out["unserved"].tolist() == [0, INT32_MAX] and out["key"][1] == timed.INT64_MAX and out["best"][0] == 0


@pytest.mark.parametrize("fn", BOTH)
def test_begin_on_the_last_layer(fn):
    """no layer is left: the robot stands; a stop on its cell is served at T without a dwell, and not with one"""
    out = one(fn, np.zeros((1, 7)), [2, 5], [2, 6], [[0], [1]], [1, 1], [0, 1], 6, begin=[6, 6])
    assert out["paths"][0].tolist() == [[2] * 7, [5] * 7] and out["status"][0].tolist() == [0, 0]
    assert out["serve_at"][0].tolist() == [[6], [-1]] and out["arrive"][0].tolist() == [6, 7] and out["unserved"][0] == 1
    out = one(fn, np.zeros((1, 7)), [2], [2], [[0]], [1], [0], 6, begin=[6], dwell=1)
    assert out["serve_at"][0, 0].tolist() == [-1] and out["arrive"][0, 0] == 7 and out["paths"][0, 0].tolist() == [2] * 7


@pytest.mark.parametrize("fn", BOTH)
def test_begin_out_of_range(fn):
    """a begin outside [0, T] skips the robot as rule 1 does; a kept robot's begin is not looked at"""
    out = one(fn, np.zeros((1, 7)), [0, 2, 4, 6], [3], [[0]] * 4, [1, 1, 1, 1], [0] * 4, 6, begin=[-1, 7, 0, 99], active=[1, 1, 1, 0])
    assert out["status"][0].tolist() == [OUTSIDE, OUTSIDE, 0, KEPT] and out["arrive"][0].tolist() == [7, 7, 1, 0]
    assert (out["paths"][0, [0, 1, 3]] == -1).all() and out["unserved"][0] == 2 and out["key"][0] == (2 << 32) | 15
    assert out["serve_at"][0, 2].tolist() == [1]        # the skipped starts on cells 0 and 2 block nobody


# ---- random problems ----------------------------------------------------------------------------------------------------
def random_problem(seed, B=None):
    rng = np.random.default_rng(1000 + seed)
    H, W = (int(v) for v in rng.integers(3, 11, 2))
    B, K = int(rng.integers(1, 6)) if B is None else B, int(rng.integers(1, 4))
    g = (rng.uniform(size=(H, W)) < rng.choice([0.0, 0.15, 0.3])).astype(float)
    free = np.flatnonzero(g.ravel() < 0.5)
    if len(free) < B + 1:
        g[:] = 0.0
        free = np.arange(H * W)
    starts = rng.choice(free, B, replace=False).astype(np.int32)
    Gf = int(rng.integers(1, 7))
    cells = rng.choice(free, Gf).astype(np.int32)
    stops = rng.integers(0, Gf, (B, K)).astype(np.int32)
    lens = rng.integers(0, K + 1, B).astype(np.int32)
    park = rng.integers(0, Gf, B).astype(np.int32)
    if seed % 9 == 0:
        starts[int(rng.integers(0, B))] = H * W                       # a skipped robot
    G = int(rng.integers(1, 3))
    orders = np.stack([rng.permutation(B) for _ in range(G)])
    if seed % 14 == 0:
        orders[-1, 0] = orders[-1, -1] if B > 1 else 1
    q = dict(grid=g, start=starts, stops=stops, lens=lens, park_index=park, goal_cells=cells, orders=orders,
             T=int(rng.integers(2, 15)), sep2=int(rng.choice([1, 2, 4, 5])), lag=int(rng.integers(1, 3)),
             dwell=int(rng.integers(0, 3)), movement=int(rng.choice([4, 8])))
    q["fields"] = fields_for(g, cells, q["movement"])
    return q, rng


def replan_inputs(q, rng, mixed=True):
    """a reserved walker or two (random walks, cells outside the map among them), a kept subset and begin layers"""
    H, W = q["grid"].shape
    T, B = q["T"], len(q["start"])
    walkers = []
    for _ in range(int(rng.integers(0, 3))):
        c, path = int(rng.integers(0, H * W)), []
        for t in range(T + 1):
            r, col = divmod(c, W)
            r, col = min(max(r + int(rng.integers(-1, 2)), 0), H - 1), min(max(col + int(rng.integers(-1, 2)), 0), W - 1)
            c = r * W + col
            path.append(-1 if rng.uniform() < 0.1 else c)
        walkers.append(path)
    active = (rng.uniform(size=B) < 0.7).astype(np.int32)
    begin = rng.integers(0, T + 1, B) if mixed else np.full(B, int(rng.integers(0, T + 1)))
    if rng.uniform() < 0.15:
        begin[int(rng.integers(0, B))] = rng.choice([-1, T + 1])
    return walkers, active, begin.astype(np.int32)


def test_restatements_agree_on_random_problems():
    seen = dict(kept=0, failed=0, served=0, clash=0, walkers=0, skipped=0)
    for seed in range(120):
        q, rng = random_problem(seed)
        walkers, active, begin = replan_inputs(q, rng)
        H, W = q["grid"].shape
        res0 = reserve_ref(H, W, q["T"], np.array(walkers), q["sep2"], q["lag"]) if walkers else None
        a = replan_ref(**q, res0=res0, active=active, begin=begin)
        b = replan_walk(**q, reserved_paths=[(p, q["sep2"]) for p in walkers], active=active, begin=begin)
        for k in OUT + ("clash",):
            assert np.array_equal(a[k], b[k]), (seed, k, a[k], b[k])
        seen["kept"] += int((a["status"] == KEPT).sum())
        seen["failed"] += int((a["status"] > 0).sum())
        seen["skipped"] += int((a["status"] == OUTSIDE).sum())
        seen["served"] += int(a["served"].sum())
        seen["clash"] += int(a["clash"].sum())
        seen["walkers"] += len(walkers)
    assert all(v > 10 for v in seen.values()), seen


def test_c1_without_a_table_all_active_from_layer_0_it_is_the_timed_tours():
    for seed in range(30):
        q, rng = random_problem(seed)
        want = plan_ref(**q)
        B = len(q["start"])
        for extra in (dict(), dict(active=np.ones(B, np.int32), begin=np.zeros(B, np.int32),
                                   res0=np.zeros((q["T"] + 1,) + q["grid"].shape, dtype=bool))):
            got = replan_ref(**q, **extra)
            for k in OUT:
                assert np.array_equal(got[k], want[k]), (seed, k)
            assert (got["clash"] == 0).all()


def test_c2_the_ranks_behind_a_kept_prefix_get_what_the_full_plan_gave_them():
    pairs = 0
    for seed in range(40):
        q, rng = random_problem(seed, B=int(2 + seed % 4))
        H, W = q["grid"].shape
        B, T = len(q["start"]), q["T"]
        full = plan_ref(**q)
        for g, order in enumerate(q["orders"]):
            if full["key"][g] == timed.INT64_MAX:
                continue
            for r in range(B + 1):
                head = [int(b) for b in order[:r]]
                if any(full["status"][g, b] == OUTSIDE for b in head):        # (a skipped robot has no path to reserve)
                    continue
                active = np.ones(B, np.int32)
                active[head] = 0
                res0 = reserve_ref(H, W, T, full["paths"][g, head], q["sep2"], q["lag"]) if head else None
                got = replan_ref(**dict(q, orders=[order]), res0=res0, active=active)
                for b in order[r:]:
                    for k in ("paths", "status", "arrive", "serve_at", "served"):
                        assert np.array_equal(got[k][0, b], full[k][g, b]), (seed, g, r, b, k)
                assert (got["status"][0, head] == KEPT).all()
                pairs += 1
    assert pairs > 150


def test_c3_a_begin_layer_is_the_shorter_window_behind_standing_layers():
    n = 0
    for seed in range(60):
        q, rng = random_problem(seed, B=1)
        if q["start"][0] >= q["grid"].size:
            continue
        T, q["orders"] = q["T"], [[0]]
        beta = int(rng.integers(0, T))
        want = plan_ref(**dict(q, T=T - beta))
        got = replan_ref(**q, begin=[beta])
        assert got["paths"][0, 0].tolist() == [int(q["start"][0])] * beta + want["paths"][0, 0].tolist()
        sa = want["serve_at"][0, 0]
        assert np.array_equal(got["serve_at"][0, 0], np.where(sa >= 0, sa + beta, -1))
        st = int(want["status"][0, 0])
        assert got["status"][0, 0] == (st + beta if st > 0 else st) and got["arrive"][0, 0] == want["arrive"][0, 0] + beta
        assert got["served"][0, 0] == want["served"][0, 0] and got["unserved"][0] == want["unserved"][0]
        n += 1
    assert n > 40


# ---- the guarantee ------------------------------------------------------------------------------------------------------
def pair_violations(W, T, sep2, lag, p, t_from, q, s_to=None):
    """the (t, s) with t > t_from, |s - t| <= lag, s <= s_to (T when None) and d2(p[t], q[s]) < sep2; a q[s] < 0 is nowhere"""
    bad = []
    for t in range(t_from + 1, T + 1):
        for s in range(max(0, t - lag), min(T if s_to is None else s_to, t + lag) + 1):
            if q[s] >= 0 and (p[t] // W - q[s] // W) ** 2 + (p[t] % W - q[s] % W) ** 2 < sep2:
                bad.append((t, s))
    return bad


def midplan_case(seed, mixed):
    """a re-plan in the middle of a full plan: begin layers, the cells the plan holds there as starts, new stops for the
    active robots, the kept robots' planned paths reserved"""
    q, rng = random_problem(seed, B=int(2 + seed % 4))
    H, W = q["grid"].shape
    B, T = len(q["start"]), q["T"]
    full = plan_ref(**q)
    g = int(full["best"][0])
    if g < 0 or (full["status"][g] != 0).any():
        return None
    begin = rng.integers(0, T, B) if mixed else np.full(B, int(rng.integers(0, T)))
    active = (rng.uniform(size=B) < 0.6).astype(np.int32)
    active[int(rng.integers(0, B))] = 1
    kept = np.flatnonzero(active == 0)
    start = full["paths"][g, np.arange(B), begin].astype(np.int32)
    res0 = reserve_ref(H, W, T, full["paths"][g, kept], q["sep2"], q["lag"]) if len(kept) else None
    new = dict(q, start=start, stops=rng.integers(0, len(q["goal_cells"]), q["stops"].shape).astype(np.int32))
    return new, full["paths"][g], kept, res0, active, begin.astype(np.int32)


@pytest.mark.parametrize("mixed", [False, True], ids=["common-begin", "mixed-begin"])
def test_c4_the_guarantee_on_midplan_replans(mixed):
    n = moved = 0
    for seed in range(70):
        case = midplan_case(seed, mixed)
        if case is None:
            continue
        q, old, kept, res0, active, begin = case
        W, T, sep2, lag = q["grid"].shape[1], q["T"], q["sep2"], q["lag"]
        out = replan_ref(**q, res0=res0, active=active, begin=begin)
        for g, order in enumerate(q["orders"]):
            if out["key"][g] == timed.INT64_MAX:
                continue
            rank = {int(b): k for k, b in enumerate(order)}
            for i in np.flatnonzero(active):
                if out["status"][g, i] != 0:
                    continue
                p = out["paths"][g, i]
                assert (p[:begin[i] + 1] == q["start"][i]).all()
                moved += int((p[begin[i]:] != p[begin[i]]).any())
                for j in kept:                                                        # any path stamped into res0
                    assert pair_violations(W, T, sep2, lag, p, begin[i], old[j]) == [], (seed, g, i, j)
                for j in np.flatnonzero(active):
                    if j == i or out["status"][g, j] == OUTSIDE:
                        continue
                    pj = out["paths"][g, j]
                    if rank[int(j)] < rank[int(i)]:                                   # the whole path of an earlier rank
                        assert pair_violations(W, T, sep2, lag, p, begin[i], pj) == [], (seed, g, i, j)
                    assert pair_violations(W, T, sep2, lag, p, begin[i], pj, s_to=begin[j]) == [], (seed, g, i, j)
        n += 1
    assert n >= 25 and moved > 20, (n, moved)


def test_c5_clash():
    n = 0
    for seed in range(160):
        case = midplan_case(seed, mixed=False)
        if case is None:
            continue
        q, old, kept, res0, active, begin = case
        W, first = q["grid"].shape[1], old[:, 0]
        if any(timed._d2(int(a), int(b), W) < q["sep2"] for i, a in enumerate(first) for b in first[:i]):
            continue                       # (starts closer than sep2 are the caller's choice: the plan is not consistent)
        assert (replan_ref(**q, res0=res0, active=active, begin=begin)["clash"] == 0).all(), seed
        n += 1
    assert n >= 25
    # a walker that stands beside a start at the robot's begin layer (and one that has left by then)
    z = np.zeros((3, 7))
    beside, gone = [8] * 10, [8, 8, 8, 9, 10, 11, 12, 13, 13, 13]
    for fn in BOTH:
        for path, begin, want in ((beside, 0, 1), (beside, 6, 1), (gone, 3, 1), (gone, 6, 0)):
            out = one(fn, z, [7, 20], [6], [[0], [0]], [0, 0], [0, 0], 9, sep2=2, reserved=[path], begin=[begin, 0])
            assert out["clash"].tolist() == [want, 0], (path, begin)
        out = one(fn, z, [7, 20], [6], [[0], [0]], [0, 0], [0, 0], 9, sep2=2, reserved=[beside], active=[0, 1])
        assert out["clash"].tolist() == [0, 0]                                       # a kept robot has no clash


# ---- the reservation table ------------------------------------------------------------------------------------------------
def test_reserve_ref_by_hand_and_the_table_words():
    res = reserve_ref(2, 70, 3, [[65, -1, 140, 69]], 2, lag=1)
    cells = lambda t: np.flatnonzero(res[t].ravel()).tolist()
    assert cells(0) == [64, 65, 66, 135] and cells(1) == cells(0)            # t = 0 reaches layer 1; t = 1 stamps nothing
    assert cells(2) == [68, 69, 139] and cells(3) == cells(2)                # 140 is outside the 2 x 70 map
    words = table_words(res).reshape(4, 2, 2)
    assert words[0].tolist() == [[0, 7], [0, 1 << 1]] and words[2].tolist() == [[0, 3 << 4], [0, 1 << 5]]
    more = reserve_ref(2, 70, 3, [[0, 0, 0, 0], [5, 5, 5, 5]], 1, use=[0, 1], res=res)
    assert np.flatnonzero(more[0].ravel()).tolist() == [5, 64, 65, 66, 135] and not res[0, 0, 5]


# ---- rebase ---------------------------------------------------------------------------------------------------------------
def test_rebase_by_hand():
    paths = np.array([[0, 1, 2, 2, 2, 3, 3], [9, 9, 9, 8, 7, 7, 7], [4, 4, 4, 4, 4, 4, 4]], np.int32)
    sa = np.array([[2, 5], [4, -1], [-1, -1]], np.int32)
    p, s, idx, begin, start, m = rebase_ref(paths, sa, [4, 3, 6], [1, 0, 0], [0, 0, 1])
    # robot 2 stands since layer 0: e = 0 holds everybody back
    assert m == 0 and np.array_equal(p, paths) and idx.tolist() == [4, 3, 0] and s.tolist() == [[-1, 5], [4, -1], [-1, -1]]
    p, s, idx, begin, start, m = rebase_ref(paths, sa, [4, 3, 6], [1, 0, 0], [1, 0, 0])
    # robot 0 is active and stands on cell 2 since layer 2; the kept robots are at 3 and 6: m = 2
    assert m == 2 and idx.tolist() == [0, 1, 4] and begin[0] == 0 and start.tolist() == [2, 8, 4]
    assert p.tolist() == [[2, 2, 2, 3, 3, 3, 3], [9, 8, 7, 7, 7, 7, 7], [4] * 7] and s.tolist() == [[-1, 3], [2, -1], [-1, -1]]


def test_rebase_on_torch_cpu_tensors_is_rebase_ref():
    import torch
    from robot_mpcs_amd.global_planner.lifelong import rebase
    rng = np.random.default_rng(5)
    shifts = 0
    for trial in range(60):
        B, T, K = int(rng.integers(1, 7)), int(rng.integers(1, 12)), int(rng.integers(1, 4))
        paths = np.cumsum(rng.integers(0, 2, (B, T + 1)), axis=1).astype(np.int32)          # runs of equal cells
        sa = np.sort(rng.integers(-1, T + 1, (B, K)), axis=1).astype(np.int32)
        idx = rng.integers(T // 2, T + 1, B).astype(np.int32)
        leg, active = rng.integers(0, K + 1, B).astype(np.int32), rng.integers(0, 2, B).astype(np.int32)
        want = rebase_ref(paths, sa, idx, leg, active)
        got = rebase(*(torch.from_numpy(a) for a in (paths, sa, idx, leg, active)))
        for a, b in zip(got[:5], want[:5]):
            assert a.dtype == torch.int32 and np.array_equal(a.numpy(), b), (trial, a, b)
        assert int(got[5]) == want[5]
        shifts += want[5] > 0
    assert shifts > 20


# ---- the header and the binding -------------------------------------------------------------------------------------------
def test_symbols_are_declared_by_the_new_header_and_exported(lib):
    from robot_mpcs_amd import _abi
    assert lib.TIMED_REPLAN_SYMBOLS == SYMBOLS == list(_abi.timed_replan_prototypes)
    check_header(lib, "rmpc_timed_replan", SYMBOLS, _abi.timed_replan_prototypes)
    vp, i = C.c_void_p, C.c_int
    S, P = _abi.timed_replan_structs["rmpc_timed_replan"], _abi.timed_tours_structs["rmpc_timed_tours"]
    assert _abi.timed_replan_prototypes[SYMBOLS[0]] == (C.c_int64, [i] * 3)
    assert _abi.timed_replan_prototypes[SYMBOLS[1]] == (i, [i, i, i, i, vp, vp, i, i, i, vp, vp])
    assert _abi.timed_replan_prototypes[SYMBOLS[2]] == (C.c_int64, [i] * 4)
    assert _abi.timed_replan_prototypes[SYMBOLS[3]] == (i, [C.POINTER(P), C.POINTER(S), vp])
    assert _abi.timed_replan_constants == {"RMPC_TIMED_RESERVE_MAX_PATHS": 4096, "RMPC_TIMED_KEPT": -9}
    assert (lib.TIMED_RESERVE_MAX_PATHS, lib.TIMED_KEPT) == (4096, KEPT)
    assert S._fields_ == [("struct_size", C.c_int32), ("res0", vp), ("active", vp), ("begin", vp), ("clash", vp), ("work", vp),
                          ("work_bytes", C.c_int64)]
    assert list(_abi.timed_replan_structs) == ["rmpc_timed_replan"] and C.sizeof(S) == 56
    # the other headers declare what they declared, and the version stands
    assert len(lib.EXPORTED_SYMBOLS) == 65 and len(lib.TIMED_TOURS_SYMBOLS) == 3 and C.sizeof(P) == 200
    assert not set(SYMBOLS) & (set(_abi.prototypes) | set(_abi.timed_tours_prototypes))


def test_the_reader_types_a_64_bit_word_and_a_struct_of_an_included_header():
    from robot_mpcs_amd import _abi
    text = "typedef struct rmpc_t { const uint64_t *w; uint64_t n; } rmpc_t;\nint rmpc_f(const rmpc_o *o, uint64_t *d_w, uint64_t *h);"
    with pytest.raises(_abi.RmpcError, match="rmpc_o"):
        _abi.parse(text)
    other = type("rmpc_o", (C.Structure,), {"_fields_": []})
    constants, structs, prototypes = _abi.parse(text, {"rmpc_o": other})
    assert structs["rmpc_t"]._fields_ == [("w", C.c_void_p), ("n", C.c_uint64)] and list(structs) == ["rmpc_t"]
    assert prototypes == {"rmpc_f": (C.c_int, [C.POINTER(other), C.c_void_p, C.POINTER(C.c_uint64)])}


def test_sizes(lib):
    L = lib.load_library()
    assert lib.timed_reserve_words(7, 5, 9) == 10 * 7 and lib.timed_reserve_words(65, 70, 40) == 41 * 65 * 2
    assert lib.timed_reserve_words(4, 130, 40) == 41 * 4 * 3 and lib.timed_reserve_words(128, 128, 1023) == 1024 * 128 * 2
    for a in ((0, 5, 9), (7, 0, 9), (129, 128, 9), (7, 5, 0), (7, 5, 1024)):
        assert L.rmpc_timed_reserve_words(*a) == -1 and L.rmpc_last_error().decode().startswith("timed reserve")
        with pytest.raises(lib.RmpcError, match="timed reserve"):
            lib.timed_reserve_words(*a)
    # the orders' parts are the timed tours'; behind them one int32 per robot of the limit, four, and three per cell
    for a in ((7, 5, 9, 2), (65, 70, 70, 3), (128, 128, 1023, 1024), (1, 1, 1, 1)):
        extra = lib.timed_replan_work_bytes(*a) - lib.timed_tours_work_bytes(*a)
        assert extra == 8 * ((1024 + 4 + 3 * a[0] * a[1] + 1) // 2)
    for a in ((0, 5, 9, 2), (129, 128, 9, 1), (7, 5, 0, 2), (7, 5, 1024, 2), (7, 5, 9, 0), (7, 5, 9, 1025)):
        assert L.rmpc_timed_replan_work_bytes(*a) == -1 and L.rmpc_last_error().decode().startswith("timed replan")
        with pytest.raises(lib.RmpcError, match="timed replan"):
            lib.timed_replan_work_bytes(*a)


PLAN = dict(H=7, W=5, movement=4, grid=P_, occ_threshold=0.8, B=3, Gf=2, start_cell=P_, K=2, dwell=1, stops=P_, len=P_,
            park_index=P_, fields=P_, goal_cells=P_, T=9, sep2=2, lag=1, G=2, orders=P_, work=None, work_bytes=0, paths=P_,
            status=P_, arrive=P_, key=P_, best=P_, serve_at=P_, served=P_, unserved=P_)
EXTRA = dict(res0=None, active=None, begin=None, clash=None, work=P_, work_bytes=1 << 20)
REFUSALS = [(dict([(k, None)]), {}, NULL) for k, v in PLAN.items() if v == P_]
REFUSALS += [(dict(K=0), {}, "timed tours: need 1 <= K"), (dict(K=65), {}, "timed tours: need 1 <= K"),
             (dict(dwell=-1), {}, "timed tours: need 0 <= dwell"), (dict(dwell=65), {}, "timed tours: need 0 <= dwell"),
             (dict(B=0), {}, "timed tours: need 1 <= B"), (dict(B=1025), {}, "timed tours: need 1 <= B"),
             (dict(T=0), {}, "timed tours: need 1 <= T"), (dict(T=1024), {}, "timed tours: need 1 <= T"),
             (dict(sep2=0), {}, "timed tours: need 1 <= sep2"), (dict(sep2=4097), {}, "timed tours: need 1 <= sep2"),
             (dict(lag=0), {}, "timed tours: lag must lie"), (dict(lag=5), {}, "timed tours: lag must lie"),
             (dict(G=0), {}, "timed tours: need 1 <= G"), (dict(G=1025), {}, "timed tours: need 1 <= G"),
             (dict(movement=6), {}, ""), (dict(H=0), {}, ""), (dict(W=0), {}, ""), (dict(H=129, W=128), {}, ""),
             (dict(Gf=0), {}, ""), (dict(Gf=I_MAX), {}, ""),
             (dict(struct_size=199), {}, "rmpc_timed_tours.struct_size mismatch"),
             ({}, dict(struct_size=55), "rmpc_timed_replan.struct_size mismatch"),
             ({}, dict(struct_size=0), "rmpc_timed_replan.struct_size mismatch"),
             ({}, dict(work=None), NULL),
             ({}, dict(work_bytes=0), "timed replan: the workspace holds 0 bytes"),
             ({}, dict(work_bytes=-1), "timed replan: the workspace holds -1 bytes")]


@pytest.mark.parametrize("bad,badx,want", REFUSALS, ids=[",".join("%s=%s" % kv for kv in {**b, **x}.items()) for b, x, _ in REFUSALS])
def test_replan_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, badx, want):
    L = lib.load_library()
    a = filled(lib.TimedToursArgs, PLAN, **bad)              # (the tours' own work is NULL: it is not read)
    x = filled(lib.TimedReplanArgs, EXTRA, **badx)
    refused(L, L.rmpc_timed_tours_replan_device(C.byref(a), C.byref(x), None), want)
    if not badx:
        assert L.rmpc_timed_tours_replan_device(None, C.byref(x), None) == -1 and L.rmpc_last_error().decode() == NULL
    assert L.rmpc_timed_tours_replan_device(C.byref(a), None, None) == -1 and L.rmpc_last_error().decode() == NULL


def test_a_workspace_one_byte_short_is_refused(lib):
    L = lib.load_library()
    a = filled(lib.TimedToursArgs, PLAN)
    x = filled(lib.TimedReplanArgs, {}, work=P_, work_bytes=lib.timed_replan_work_bytes(7, 5, 9, 2) - 1)
    assert L.rmpc_timed_tours_replan_device(C.byref(a), C.byref(x), None) == -1
    assert "are needed (rmpc_timed_replan_work_bytes)" in L.rmpc_last_error().decode()


RESERVE = dict(H=7, W=5, T=9, P=3, cells=P_, use=None, sep2=2, lag=1, clear=1, res=P_, stream=None)
RESERVE_REFUSALS = [(dict(cells=None), NULL), (dict(res=None), NULL), (dict(P=0), "timed reserve: need 1 <= P"),
                    (dict(P=4097), "timed reserve: need 1 <= P <= RMPC_TIMED_RESERVE_MAX_PATHS = 4096"),
                    (dict(T=0), "timed reserve: need 1 <= T"), (dict(T=1024), "timed reserve: need 1 <= T"),
                    (dict(sep2=0), "timed reserve: need 1 <= sep2"), (dict(sep2=4097), "timed reserve: need 1 <= sep2"),
                    (dict(lag=0), "timed reserve: lag must lie"), (dict(lag=5), "timed reserve: lag must lie"),
                    (dict(H=0), ""), (dict(W=0), ""), (dict(H=129, W=128), "")]


@pytest.mark.parametrize("bad,want", RESERVE_REFUSALS, ids=[",".join("%s=%s" % kv for kv in b.items()) for b, _ in RESERVE_REFUSALS])
def test_reserve_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    L = lib.load_library()
    assert L.rmpc_timed_reserve_device(*dict(RESERVE, **bad).values()) == -1
    msg = L.rmpc_last_error().decode()
    assert msg.startswith(want) and msg, (msg, want)


# ---- a kinematic lifelong walk --------------------------------------------------------------------------------------------
WALK_SEED, WALK_EVERY = 0, 14      # the first seed and wave spacing tried for which the restatements alone serve every pick


def test_kinematic_lifelong_walk_serves_three_waves_and_keeps_the_robots_apart():
    """5 robots on a 12 x 12 map with two shelves, 6 picks and then two further waves of 5 picks every WALK_EVERY steps,
    through ``start_ref`` / ``dispatch_ref`` (rebase, tours on +inf rows, reserve, re-plan, merge) and ``follow_ref``.
    Every robot moves 0.8 of the way to its goal per step; robot 0 stands still for its first 6 steps.  Every pick of
    every wave is served, no plan fails, clash is 0, and no two robots are ever closer than sep2 (in cells, each robot on
    the cell nearest to it) at the same step."""
    from timed_replan_reference import dispatch_ref, start_ref
    from timed_tours_reference import follow_ref
    rng = np.random.default_rng(WALK_SEED)
    H = W = 12
    grid = np.zeros((H, W))
    grid[3:5, 2:6] = grid[7:9, 6:10] = 1.0
    K, T, sep2, lag, dwell, B = 2, 80, 4, 1, 1, 5
    orders = np.stack([np.arange(B), np.arange(B)[::-1]])
    free = np.flatnonzero(grid.ravel() < 0.5)

    def spaced(n, apart, avoid=()):
        out = []
        while len(out) < n:
            c = int(rng.choice(free))
            if all(timed._d2(c, q, W) >= apart for q in list(out) + list(avoid)):
                out.append(c)
        return np.array(out, np.int32)
    starts = spaced(B, 9)
    waves = [spaced(6, sep2, starts)] + [spaced(5, sep2) for _ in range(2)]
    state, left = start_ref(grid, starts, waves[0], K, T, sep2, lag, dwell, orders)
    total, served_total = len(waves[0]) - len(left), 0
    pos = np.stack([starts % W, starts // W], 1).astype(float)
    goal = np.zeros((B, 3))
    served = np.full((B, K), -1, np.int32)
    for step in range(3 * WALK_EVERY + 2 * T):
        wave = step // WALK_EVERY
        if step % WALK_EVERY == 0 and 1 <= wave <= 2:
            picks = np.concatenate([left, waves[wave]]).astype(np.int32)
            active = (state["leg"] >= state["nstops"]) & (state["paths"][np.arange(B), state["idx"]] == state["paths"][:, T])
            served_total += int((served[active] >= 0).sum())
            left = dispatch_ref(grid, state, picks, K, T, sep2, lag, dwell, orders)
            served[active] = -1
            total += len(picks) - len(left)
        state["idx"], goal, blk, state["leg"], served = follow_ref(state["paths"], state["idx"], pos, goal, W, 0.0, 0.0, 1.0, 0.3,
                                                                   sep2, lag, state["serve_at"], state["leg"], served, step, 0.3)
        move = np.full((B, 1), 0.8)
        if step < 6:
            move[0] = 0.0
        pos += move * (goal[:, :2] - pos)
        cells = np.rint(pos[:, 1]).astype(int) * W + np.rint(pos[:, 0]).astype(int)
        assert all(timed._d2(int(a), int(b), W) >= sep2 for i, a in enumerate(cells) for b in cells[:i]), (step, cells)
        if wave >= 2 and served_total + int((served >= 0).sum()) == total and len(left) == 0:
            break
    assert len(left) == 0 and total == 16 and served_total + int((served >= 0).sum()) == 16, (left, total, served)
    assert state["failures"] == 0 and state["clash"] == 0
