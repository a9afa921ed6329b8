"""Lifelong timed tours on the device (rmpc_timed_reserve_device, rmpc_timed_tours_replan_device,
include/rmpc_timed_replan.h) against the numpy restatement of tests/timed_replan_reference.py, bit for bit;
every launch writes into poisoned outputs and a workspace of 0xA5.  The restatement ranks end cells on the fields the
device computed, so that both compare the same doubles.  The shapes are those of tests/test_gpu_timed_tours.py: the
smallest that reach each code path."""
import numpy as np
import pytest

from example_loader import load_example
from gpu_support import DEV, _t
from timed_cases import random_tours_case as _random_case, walkers as _walkers
from timed_reference import BAD_ORDER, OUTSIDE
from timed_replan_reference import KEPT, rebase_ref, replan_ref, reserve_ref, table_words
from timed_support import load_runtime, poisoned, same, stage, workspace
from timed_tours_reference import INT32_MAX, store_tours_case

pytestmark = pytest.mark.gpu

KEYS = ("paths", "status", "arrive", "serve_at", "served", "key", "unserved", "best", "clash")


@pytest.fixture(scope="module")
def rt():
    return load_runtime()


def _device_reserve(rt, H, W, T, cells, sep2, lag=1, use=None, res=None, stream=None):
    """-> the table's words as uint64; ``res``: a device table to OR into (clear = 0), None = a poisoned one, cleared"""
    torch, lib = rt["torch"], rt["lib"]
    d_cells = _t(torch, np.asarray(cells, np.int32).reshape(-1, T + 1), torch.int32)
    d_use = None if use is None else _t(torch, np.asarray(use), torch.int32)
    clear = res is None
    if res is None:
        res = torch.full((lib.timed_reserve_words(H, W, T),), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    lib.timed_reserve_device(d_cells, res, H, W, sep2, lag, use=d_use, clear=clear, stream=stream)
    torch.cuda.synchronize()
    return res, res.cpu().numpy().view(np.uint64)


def _staged(rt, grid, starts, cells, stops, lens, park, orders, T, movement, occ, stream, keys):
    """the case on the device, and poisoned outputs ``keys`` for it"""
    stops = np.asarray(stops, dtype=np.int32).reshape(len(starts), -1)
    d = stage(rt, grid, cells, orders, movement, occ, stream, starts=starts, stops=stops, lens=lens, park=park)
    G, B = d["orders"].shape
    return d, poisoned(rt["torch"], keys, G, B, T, stops.shape[1])


def _tours_args(lib, d, out, work, sep2, lag, dwell, movement, occ):
    return lib.timed_tours_args(d["grid"], d["starts"], d["stops"], d["lens"], d["park"], d["fields"], d["cells"], d["orders"],
                                work, out["paths"], out["status"], out["arrive"], out["key"], out["best"], out["serve_at"],
                                out["served"], out["unserved"], dwell=dwell, movement=movement, occ_threshold=occ, sep2=sep2,
                                lag=lag)


def _device_tours_plan(rt, grid, starts, cells, stops, lens, park, orders, T, sep2, lag=1, dwell=0, movement=4, occ=0.8):
    """rmpc_timed_tours_plan_device on the same case -> its results as numpy"""
    torch, lib = rt["torch"], rt["lib"]
    d, out = _staged(rt, grid, starts, cells, stops, lens, park, orders, T, movement, occ, None, KEYS[:-1])
    (G, B), (H, W) = d["orders"].shape, d["grid"].shape
    work = workspace(torch, lib.timed_tours_work_bytes(H, W, T, G))
    lib.timed_tours_plan_device(_tours_args(lib, d, out, work, sep2, lag, dwell, movement, occ))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _device_replan(rt, grid, starts, cells, stops, lens, park, orders, T, sep2, lag=1, dwell=0, movement=4, occ=0.8, res0=None,
                   active=None, begin=None, stream=None, work=None, restate=True):
    """-> (device results as numpy, the restatement's) for the same fields; res0: boolean layers or None"""
    torch, lib = rt["torch"], rt["lib"]
    d, out = _staged(rt, grid, starts, cells, stops, lens, park, orders, T, movement, occ, stream, KEYS)
    (G, B), (H, W) = d["orders"].shape, d["grid"].shape
    if work is None:
        work = workspace(torch, lib.timed_replan_work_bytes(H, W, T, G))
    args = _tours_args(lib, d, out, work[:0], sep2, lag, dwell, movement, occ)
    args.work, args.work_bytes = None, 0                   # (not read)
    d_res = None if res0 is None else _t(torch, table_words(res0).view(np.int64), torch.int64)
    opt = lambda a: None if a is None else _t(torch, np.asarray(a), torch.int32)
    x = lib.timed_replan_args(work, d_res, opt(active), opt(begin), out["clash"])
    lib.timed_tours_replan_device(args, x, stream=stream)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    want = replan_ref(np.asarray(grid, dtype=float), starts, stops, lens, park, d["fields"].cpu().numpy(),
                      np.asarray(cells, dtype=np.int32), orders, T, sep2, lag, dwell, movement, occ, res0=res0, active=active,
                      begin=begin) if restate else None
    return got, want


def _same(got, want, keys=KEYS):
    same(got, want, keys)


SHAPES = [
    ("small", 7, 5, 3, 9, 2, 2, 4, 1, 2, 1),
    ("eight-moves-lag-2-dwell-0", 12, 9, 5, 20, 2, 3, 8, 2, 4, 0),
    ("eight-moves-lag-2-dwell-1", 12, 9, 5, 20, 2, 3, 8, 2, 4, 1),
    ("eight-moves-lag-2-dwell-3", 12, 9, 5, 20, 2, 3, 8, 2, 4, 3),
    ("word-and-lane-seams", 65, 70, 6, 40, 2, 2, 8, 1, 5, 2),          # two words per row; the history in LDS
    ("history-in-the-workspace", 65, 70, 6, 70, 2, 2, 4, 1, 5, 2),     # 71 layers of 130 words: beyond the history's LDS
    ("three-words-per-row", 4, 130, 4, 40, 2, 2, 8, 1, 4, 1),
    ("128-threads", 100, 20, 4, 30, 2, 2, 4, 3, 10, 1),                # 100 words per layer
]


# ---- the reservation table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,H,W,B,T,G,K,movement,lag,sep2,dwell", SHAPES)
def test_reserve_is_the_restatement(rt, name, H, W, B, T, G, K, movement, lag, sep2, dwell):
    rng = np.random.default_rng(3 * H + W + T)
    cells = _walkers(rng, H, W, T, 5)
    cells[0, ::3] = [-1, H * W, -7][T % 3]                               # cells outside the map stamp nothing
    use = np.array([1, 0, 2, 1, -1], np.int32)
    res, got = _device_reserve(rt, H, W, T, cells, sep2, lag, use=use)
    want = reserve_ref(H, W, T, cells, sep2, lag, use=use)
    assert np.array_equal(got, table_words(want)) and want.any()
    past = np.uint64(0) if W % 64 == 0 else ~np.uint64(0) << np.uint64(W % 64)      # no bit past column W - 1
    assert not (got.reshape(T + 1, H, -1)[:, :, -1] & past).any()
    # a second call with a wider sep2 ORs into what is there; without d_use every row counts
    more = _walkers(rng, H, W, T, 2)
    _, got2 = _device_reserve(rt, H, W, T, more, sep2 + 5, lag, res=res)
    want2 = reserve_ref(H, W, T, more, sep2 + 5, lag, res=want)
    assert np.array_equal(got2, table_words(want2)) and want2.sum() > want.sum()
    assert not (got2.reshape(T + 1, H, -1)[:, :, -1] & past).any()


def test_reserve_of_the_most_paths_and_the_widest_disc(rt):
    rng = np.random.default_rng(1)
    cells = _walkers(rng, 9, 66, 6, 4096)
    _, got = _device_reserve(rt, 9, 66, 6, cells, 2, 1)
    assert np.array_equal(got, table_words(reserve_ref(9, 66, 6, cells, 2, 1)))
    one = np.array([[0, 65, 9 * 66 - 1, -1, 300, 300, 4]], np.int32)
    _, got = _device_reserve(rt, 9, 66, 6, one, 4096, 4)                  # a disc wider than the map, the longest lag
    assert np.array_equal(got, table_words(reserve_ref(9, 66, 6, one, 4096, 4)))


# ---- the re-plan -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,H,W,B,T,G,K,movement,lag,sep2,dwell", SHAPES)
def test_replan_is_the_restatement(rt, name, H, W, B, T, G, K, movement, lag, sep2, dwell):
    c, rng = _random_case(H, W, B, K, 7 * H + W + T, sep2=sep2)
    orders = [np.arange(B)] + [rng.permutation(B) for _ in range(G - 1)]
    res0 = reserve_ref(H, W, T, _walkers(rng, H, W, T, 3), sep2, lag)
    seen = dict(kept=0, planned=0, served=0, late_begin=0)
    for trial in range(3):                                 # random kept subsets and mixed begin layers
        active = (rng.uniform(size=B) < 0.7).astype(np.int32)
        active[trial % B] = 1
        begin = rng.integers(0, [1, T // 2, T + 1][trial], B).astype(np.int32)
        got, want = _device_replan(rt, orders=orders, T=T, sep2=sep2, lag=lag, dwell=dwell, movement=movement,
                                   res0=res0 if trial else None, active=active, begin=begin, **c)
        _same(got, want)
        seen["kept"] += int((got["status"] == KEPT).sum())
        seen["planned"] += int((got["status"] >= 0).sum())
        seen["served"] += int(got["served"].sum())
        seen["late_begin"] += int((begin[active != 0] > lag).sum())
    assert seen["planned"] > 0 and seen["served"] > 0 and seen["late_begin"] > 0, seen


def test_hand_cases(rt):
    z = np.zeros((1, 7))
    kept = reserve_ref(1, 7, 9, [[3, 3, 3, 4, 5, 6, 6, 6, 6, 6]], 1, 1)
    got, want = _device_replan(rt, z, [0, 3], [4], [[0], [0]], [1, 0], [0, 0], [[0, 1]], 9, 1, res0=kept, active=[1, 0])
    _same(got, want)                                                     # the corridor: a wait for the kept robot
    assert got["paths"][0, 0].tolist() == [0, 1, 2, 2, 3, 4, 4, 4, 4, 4] and got["status"][0].tolist() == [0, KEPT]
    for order in ([0, 1], [1, 0]):                                        # a start is held until its begin layer + lag
        got, want = _device_replan(rt, z, [3, 0], [3, 6], [[0], [0]], [0, 1], [1, 0], [order], 9, 1, begin=[3, 0])
        _same(got, want)
        assert got["paths"][0].tolist() == [[3, 3, 3, 3, 4, 5, 6, 6, 6, 6], [0, 1, 2, 2, 2, 3, 3, 3, 3, 3]]
    got, want = _device_replan(rt, z, [2, 5], [2, 6], [[0], [1]], [1, 1], [0, 1], [[0, 1]], 6, 1, begin=[6, 6])
    _same(got, want)                                                     # begin == T
    assert got["serve_at"][0].tolist() == [[6], [-1]] and got["paths"][0].tolist() == [[2] * 7, [5] * 7]
    got, want = _device_replan(rt, z, [0, 2, 4, 6], [3], [[0]] * 4, [1] * 4, [0] * 4, [np.arange(4)], 6, 1, begin=[-1, 7, 0, 99],
                               active=[1, 1, 1, 0])
    _same(got, want)                                                     # begin out of range
    assert got["status"][0].tolist() == [OUTSIDE, OUTSIDE, 0, KEPT] and got["key"][0] == (2 << 32) | 15
    walker = reserve_ref(3, 7, 9, [[8] * 10], 2, 1)
    got, want = _device_replan(rt, np.zeros((3, 7)), [7, 20], [6], [[0], [0]], [0, 0], [0, 0], [[0, 1]], 9, 2, res0=walker)
    _same(got, want)                                                     # a walker stands beside a start
    assert got["clash"].tolist() == [1, 0]


@pytest.mark.parametrize("H,W,B,T,K,movement,lag,sep2,dwell", [(7, 5, 3, 9, 2, 4, 1, 2, 1), (12, 9, 5, 20, 3, 8, 2, 4, 1),
                                                               (65, 70, 6, 70, 2, 4, 1, 5, 2)])
def test_c1_and_c2_against_the_timed_tours_entry_itself(rt, H, W, B, T, K, movement, lag, sep2, dwell):
    torch, lib = rt["torch"], rt["lib"]
    c, rng = _random_case(H, W, B, K, 7 * H + W + T, sep2=sep2)
    orders = np.stack([np.arange(B), rng.permutation(B)]).astype(np.int32)
    full = _device_tours_plan(rt, orders=orders, T=T, sep2=sep2, lag=lag, dwell=dwell, movement=movement, **c)
    # C1: no table, all active, begin 0
    for extra in (dict(), dict(active=np.ones(B, np.int32), begin=np.zeros(B, np.int32))):
        got, _ = _device_replan(rt, orders=orders, T=T, sep2=sep2, lag=lag, dwell=dwell, movement=movement, restate=False,
                                **extra, **c)
        _same(got, full, KEYS[:-1])
        assert (got["clash"] == 0).all()
    # C2: the first r ranks kept and their planned paths reserved on the device
    for g, order in enumerate(orders):
        for r in range(1, B + 1):
            head = order[:r]
            active = np.ones(B, np.int32)
            active[head] = 0
            _, words = _device_reserve(rt, H, W, T, full["paths"][g, head], sep2, lag)
            res0 = reserve_ref(H, W, T, full["paths"][g, head], sep2, lag)
            assert np.array_equal(words, table_words(res0))
            got, _ = _device_replan(rt, orders=[order], T=T, sep2=sep2, lag=lag, dwell=dwell, movement=movement, res0=res0,
                                    active=active, restate=False, **c)
            for b in order[r:]:
                for k in ("paths", "status", "arrive", "serve_at", "served"):
                    assert np.array_equal(got[k][0, b], full[k][g, b]), (g, r, b, k)
            assert (got["status"][0, head] == KEPT).all() and (got["paths"][0, head] == -1).all()


def test_a_kept_robot_of_each_kind(rt):
    """kept robots that rule 1 would skip, whose begin is out of range, and that are planned otherwise: all KEPT, none
    counted, none in a mask"""
    g = np.zeros((4, 4))
    starts = [0, -1, 3, 12, 15, 16, 5]
    stops = [[0, 1], [0, 1], [0, 2], [0, 1], [1, -1], [0, 1], [0, 1]]
    got, want = _device_replan(rt, g, starts, [5, 10], stops, [2, 1, 2, 3, 2, -1, 2], [1, 1, 1, 1, 0, 2, 0],
                               [np.arange(7), np.arange(7)[::-1]], 9, 1, active=[1, 0, 0, 1, 0, 0, 0], begin=[0, 0, 0, 0, 50, 0, 2])
    _same(got, want)
    assert got["status"][0].tolist() == [0, KEPT, KEPT, OUTSIDE, KEPT, KEPT, KEPT]
    assert (got["arrive"][:, [1, 2, 4, 5, 6]] == 0).all() and (got["serve_at"][:, 1:] == -1).all()


def test_rows_that_are_no_permutations(rt):
    c, rng = _random_case(7, 5, 3, 2, 3, sep2=2)
    got, want = _device_replan(rt, orders=[[0, 1, 2], [0, 3, 1], [2, 1, 0]], T=9, sep2=2, dwell=1, active=[1, 0, 1], begin=[2, 0, 0],
                               **c)
    _same(got, want)
    assert got["status"][1].tolist() == [BAD_ORDER] * 3 and got["unserved"][1] == INT32_MAX and got["best"][0] in (0, 2)
    got, want = _device_replan(rt, orders=[[1, 1, 0], [-1, 0, 1]], T=9, sep2=2, dwell=1, active=[1, 0, 1], **c)
    _same(got, want)
    assert got["best"][0] == -1


def test_twice_on_one_workspace_and_on_a_side_stream(rt):
    torch, lib = rt["torch"], rt["lib"]
    c, rng = _random_case(12, 9, 5, 3, 21)
    orders = [np.arange(5), rng.permutation(5)]
    res0 = reserve_ref(12, 9, 20, _walkers(rng, 12, 9, 20, 2), 4, 1)
    kw = dict(orders=orders, T=20, sep2=4, dwell=1, movement=8, res0=res0, active=[1, 1, 0, 1, 1], begin=[0, 3, 0, 7, 1])
    work = workspace(torch, lib.timed_replan_work_bytes(12, 9, 20, 2))
    a, want = _device_replan(rt, work=work, **kw, **c)
    _same(a, want)
    b, _ = _device_replan(rt, work=work, restate=False, **kw, **c)        # what the first left in it
    _same(b, a)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # (the copies of the inputs run on it too)
        s, _ = _device_replan(rt, stream=side.cuda_stream, restate=False, **kw, **c)
        _, words = _device_reserve(rt, 12, 9, 20, a["paths"][0, :2], 4, 1, stream=side.cuda_stream)
    _same(s, a)
    assert np.array_equal(words, table_words(reserve_ref(12, 9, 20, a["paths"][0, :2], 4, 1)))


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def test_assign_with_available_is_the_tours_rule_on_inf_rows(rt):
    import tours_reference
    from assignment_reference import route_costs_ref
    from global_planner_reference import field_ref
    torch = rt["torch"]
    from robot_mpcs_amd.global_planner import TourPlanner
    c, rng = _random_case(12, 9, 5, 2, 4, density=0.1)
    goals = c["cells"][:7]
    available = np.array([1, 0, 1, 0, 1], np.int32)
    tp = TourPlanner(_t(torch, c["grid"]), goals, 2)
    tours, lens = tp.assign(_t(torch, c["starts"], torch.int32), available=_t(torch, available, torch.int32))
    torch.cuda.synchronize()
    fields = np.stack([field_ref(c["grid"], int(g)) for g in goals])
    start_cost = route_costs_ref(c["grid"], fields, c["starts"])
    start_cost[available == 0] = np.inf
    want = tours_reference.tours_problem_ref(start_cost, route_costs_ref(c["grid"], fields, goals), 2)
    assert np.array_equal(tours.cpu().numpy(), want["tours"]) and np.array_equal(lens.cpu().numpy(), want["len"])
    assert (want["len"][available == 0] == 0).all() and want["len"].sum() > 0
    tours, lens = tp.assign(_t(torch, c["starts"], torch.int32))                       # None: as before
    torch.cuda.synchronize()
    start_cost = route_costs_ref(c["grid"], fields, c["starts"])
    want = tours_reference.tours_problem_ref(start_cost, route_costs_ref(c["grid"], fields, goals), 2)
    assert np.array_equal(tours.cpu().numpy(), want["tours"]) and np.array_equal(lens.cpu().numpy(), want["len"])


def test_follower_replace(rt):
    torch = rt["torch"]
    from robot_mpcs_amd.global_planner import TimedTourFollower
    i32 = torch.int32
    fol = TimedTourFollower(_t(torch, [[0, 1, 2, 2]], i32), _t(torch, [[2]], i32), 5, 0.0, 0.0, 1.0, 0.3, 0.1, 1, 1)
    pos, goal = _t(torch, [[0.0, 0.0]]), _t(torch, np.zeros((1, 3)))
    fol.step(pos, goal)
    fol.replace(_t(torch, [[3, 3, 4, 4]], i32), _t(torch, [[3]], i32), _t(torch, [1], i32), _t(torch, [0], i32))
    fol.step(_t(torch, [[3.0, 0.0]]), goal)
    torch.cuda.synchronize()
    assert fol.idx.tolist() == [2] and goal[0].tolist() == [4.0, 0.0, 0.0] and fol.now == 2 and fol.served.tolist() == [[-1]]


@pytest.fixture(scope="module")
def dispatched(rt):
    """the store case of tests/test_gpu_timed_tours.py through ``LifelongTours``: the first wave, the followers put at
    layer L by hand (half of the robots have served their stops and stand parked by then), 16 new picks dispatched to
    the idle ones -- and the composed restatements on the device's fields"""
    import tours_reference
    from assignment_reference import route_costs_ref
    torch = rt["torch"]
    from robot_mpcs_amd.global_planner import LifelongTours, priority_orders
    from robot_mpcs_amd.store import STORE as S
    raw, g_inf, starts, picks = store_tours_case(16, 40, 0, 9)
    picks, new = picks[:24], picks[24:]
    assert np.array_equal(picks, store_tours_case(16, 24, 0, 9)[3])
    ll = LifelongTours(g_inf, 2, 255, 9, 1, 3, 16, W=S.W, x0=S.x0, y0=S.y0, cell=S.cell, threshold=0.3, stop_tol=0.1, device=DEV)
    assert len(ll.start(starts, picks)) == 0
    fol = ll.follower
    p0, sa0 = fol.paths.cpu().numpy(), fol.serve_at.cpu().numpy()
    L = int(np.sort(sa0.max(1))[7]) + 1                       # the eighth robot has just reached its last stop
    idx = np.full(16, L, np.int32)
    leg = ((sa0 >= 0) & (sa0 < L)).sum(1).astype(np.int32)
    idle = ((leg >= (sa0 >= 0).sum(1)) & (p0[:, L] == p0[:, -1])).astype(np.int32)
    fol.idx, fol.leg = _t(torch, idx, torch.int32), _t(torch, leg, torch.int32)
    left = ll.dispatch(new, "idle")
    torch.cuda.synchronize()
    host = lambda v: v.cpu().numpy() if torch.is_tensor(v) else v
    last = {k: tuple(host(a) for a in v) if isinstance(v, tuple) else host(v) for k, v in ll.last.items()}
    # the restatements, composed
    p1, sa1, idx1, begin, start, m = rebase_ref(p0, sa0, idx, leg, idle)
    fields = last["fields"]
    start_cost = route_costs_ref(g_inf, fields[:16], start)
    start_cost[idle == 0] = np.inf
    tours = tours_reference.tours_problem_ref(start_cost, route_costs_ref(g_inf, fields[:16], new), 2)
    lens = tours["len"].astype(np.int32)
    goal_cells = np.concatenate([new, np.repeat(start, 2), start]).astype(np.int32)
    park = np.where(lens > 0, tours["tours"][np.arange(16), np.maximum(lens, 1) - 1], 16 + 32 + np.arange(16)).astype(np.int32)
    res0 = reserve_ref(S.H, S.W, 255, p1, 9, 1, use=1 - idle)
    want = replan_ref(g_inf, start, np.maximum(tours["tours"], 0), lens, park, fields, goal_cells, priority_orders(16, 16, 0), 255,
                      9, 1, 3, 8, res0=res0, active=idle, begin=begin)
    return dict(ll=ll, last=last, want=want, idle=idle, rebased=(p1, sa1, idx1, begin, start, m), tours=tours, leg=leg,
                goal_cells=goal_cells, park=park, left=left, new=new, L=L)


def test_dispatch_is_the_composed_restatements(rt, dispatched):
    d = dispatched
    last, want, idle, (p1, sa1, idx1, begin, start, m) = d["last"], d["want"], d["idle"], d["rebased"]
    assert 8 <= idle.sum() < 16                               # robots of both kinds (a robot idle since layer 0 holds m at 0)
    assert np.array_equal(last["active"], idle) and np.array_equal(last["begin"], begin) and np.array_equal(last["start"], start)
    assert int(last["m"]) == m and all(np.array_equal(a, b) for a, b in zip(last["rebased"], (p1, sa1, idx1)))
    assert np.array_equal(last["tours"], d["tours"]["tours"]) and np.array_equal(last["tour_len"], d["tours"]["len"])
    assert np.array_equal(last["goal_cells"], d["goal_cells"]) and np.array_equal(last["park"], d["park"])
    for k in KEYS[:-2]:
        assert np.array_equal(last[k], want[k]), k
    g = int(want["best"][0])
    ll, on = d["ll"], idle.astype(bool)
    fol = ll.follower
    assert last["best"] == g and np.array_equal(ll.clash.cpu().numpy(), want["clash"])
    assert np.array_equal(fol.paths.cpu().numpy(), np.where(on[:, None], want["paths"][g], p1))
    assert np.array_equal(fol.serve_at.cpu().numpy(), np.where(on[:, None], want["serve_at"][g], sa1))
    assert np.array_equal(fol.idx.cpu().numpy(), idx1) and np.array_equal(fol.leg.cpu().numpy(), np.where(on, 0, d["leg"]))
    assert np.array_equal(ll.nstops.cpu().numpy()[on], want["served"][g][on])
    # the picks that are left: without an owner, or not served in the window
    placed = {int(d["new"][t]) for b in np.flatnonzero(on) for t in d["tours"]["tours"][b, :want["served"][g, b]]}
    assert sorted(d["left"].tolist()) == sorted(set(d["new"].tolist()) - placed) and len(placed) >= idle.sum()


def test_the_merged_plan_keeps_the_guarantee(dispatched):
    from robot_mpcs_amd.store import STORE as S
    from timed_reference import conflicts
    ll, want = dispatched["ll"], dispatched["want"]
    g = int(want["best"][0])
    assert int(ll.clash_sum.item()) == 0 and (want["status"][g][dispatched["idle"] != 0] == 0).all()
    assert conflicts(ll.follower.paths.cpu().numpy(), np.zeros(16, int), S.W, 9, 1) == []


# ---- closed loop -------------------------------------------------------------------------------------------------------
def test_closed_loop_lifelong(rt):
    """16 boxers in the store (examples/fleet_store_lifelong.py, seed 0, K = 2, dwell 3, 16 orders): 24 picks, then two
    further waves of 16 picks, 16 control steps apart -- part of the fleet is still on its first tour --, dispatched to
    the idle robots around the reserved routes of the others.  The gates are
    those of test_closed_loop_timed_tours: every planned pick of every wave is served within 400 control steps of the
    last dispatch, at most 1 % of the robot-steps failed, no base centre inside a shelf, no pair of end links closer
    than r_i + r_j - 1e-3 m, every robot stood at least ``dwell`` consecutive steps on each of its picks, no plan
    failure, and the sum of clash is 0.  The steps, the gaps and the figures of ``all`` and ``static`` are in DESIGN.md
    26, not asserted."""
    ex = load_example("fleet_store_lifelong")
    out = ex.run(waves=2, every=16, steps=400, seed=0, replan="idle", dwell=3)
    print(out)
    assert out["plan_failures"] == 0 and out["clash_sum"] == 0, out
    assert len(out["picks_planned"]) == 3 and min(out["picks_planned"]) > 0, out
    assert out["picks_served_total"] == sum(out["picks_planned"]), out
    assert out["steps_after_last_dispatch"] <= 400, out
    assert out["failed_share"] <= 0.01, out
    assert out["base_inside"] == 0 and out["min_base_clearance_m"] > 0.0, out
    assert out["min_pair_gap_m"] >= -1e-3, out
    assert out["min_steps_on_a_pick"] >= 3, out
