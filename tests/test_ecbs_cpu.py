"""Focal conflict-based search over the timed routes (include/rmpc_ecbs.h), what needs no GPU: the
restatement ``ecbs_ref`` on hand-worked focal routes, against ``cbs_ref`` and the exhaustive ``joint_optimum``, the
properties (a) to (e) of the header, the batch sizes and the slices, the stops short of a solution, the store with four
robots, and the header, the binding and the entry's refusals.  tests/test_gpu_ecbs.py holds the device to the
restatement."""
import ctypes as C
import itertools

import numpy as np
import pytest

from cbs_cases import CASES as CBS_CASES, HAND, problem
from cbs_reference import INF, INFEASIBLE, POOL, ROUNDS, SOLVED, CbsSearch, cbs_ref, joint_optimum
from ecbs_cases import CASES, MANY, STORE4, WEIGHTS, key
from ecbs_reference import INFO, EcbsSearch, ecbs_ref
from test_cbs_cpu import small_problems
from timed_reference import conflicts, fields_for, plan_ref, store_case
from timed_support import I_MAX, NULL, P_, check_header, filled, load_lib, refused

SYMBOLS = ["rmpc_ecbs_work_bytes", "rmpc_ecbs_device"]
OUT = ("paths", "status", "arrive", "info")


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def run(case, **over):
    """``ecbs_ref`` on a case of tests/ecbs_cases.py, with its numbers overridden by name"""
    c = dict(case, **over)
    goal_cells, gi = problem(c)
    fields = fields_for(c["grid"], goal_cells, c["movement"])
    return ecbs_ref(c["grid"], c["starts"], gi, fields, goal_cells, c["T"], c["sep2"], c["lag"], c["movement"],
                    nodes=c["nodes"], expand=c["expand"], rounds=c["rounds"], slices=c.get("slices"), w=c.get("w", (1, 1)))


def run_cbs(c):
    goal_cells, gi = problem(c)
    fields = fields_for(c["grid"], goal_cells, c["movement"])
    return cbs_ref(c["grid"], c["starts"], gi, fields, goal_cells, c["T"], c["sep2"], c["lag"], c["movement"],
                   nodes=c["nodes"], expand=c["expand"], rounds=c["rounds"])


@pytest.fixture(scope="module")
def results():
    """every shared case once"""
    return {name: run(c) for name, c in CASES.items()}


@pytest.fixture(scope="module")
def small():
    """the 48 small problems of tests/test_cbs_cpu.py (the same ``random_case`` calls) with their joint optimum"""
    out = []
    for c in small_problems():
        goal_cells, gi = problem(c)
        out.append((c, joint_optimum(c["grid"], c["starts"], gi, goal_cells, c["T"], c["sep2"], c["lag"], c["movement"])))
    return out


# ---- hand-worked focal routes -----------------------------------------------------------------------------------------
# A free 3 x 5 map, cells row * 5 + col, four moves in the order (from the left, from above, from the right, from below),
# sep2 1 (only the same cell conflicts), lag 1, T 6.  Robot b goes from 5 (row 1, col 0) to g = 8 (row 1, col 3): three
# moves along row 1, so a = 3 and p = 5 6 7 8 8 8 8 -- every other way leaves the row and costs two moves more.
def _focal(other, w):
    s = EcbsSearch(np.zeros((3, 5)), [5, int(other[0])], [0, 1], fields_for(np.zeros((3, 5)), [8, int(other[-1])], 4),
                   [8, int(other[-1])], 6, 1, 1, 4, w=w)
    empty = np.zeros((7, 3, 5), dtype=bool)
    other = np.asarray(other, dtype=np.int32)
    return s, s.focal_route(0, empty, [other]), s.penalty([other])


CROSSING = [2, 7, 12, 12, 12, 12, 12]       # the other robot comes down column 2: on 7, in b's row, at layer 1


def _crossing_penalty():
    """pen of CROSSING by hand.  (j, s) counts for the layers t with |t - s| <= 1 but for (t, s) = (0, 0).  Cell 2 is held
    at s = 0: layer 1 (layer 0 is exempt).  Cell 7 at s = 1: layers 0, 1, 2.  Cell 12 at s = 2 .. 6: layer 1 sees s = 2;
    layer 2 sees 2, 3; layers 3, 4, 5 see three each; layer 6 sees 5, 6."""
    pen = np.zeros((7, 3, 5), dtype=np.int64)
    pen[1, 0, 2] = 1
    pen[0:3, 1, 2] = 1
    pen[1:7, 2, 2] = [1, 2, 3, 3, 3, 2]
    return pen


def test_focal_route_waits_a_layer_when_that_saves_a_conflict_and_w_allows_it():
    """w = 3/2: A = min(6, floor(3 * 3 / 2)) = 4, the candidates are a2 = 3 and a2 = 4; pen is 0 on g = 8 in every layer,
    so hold = 0.  c[0][5] = 0; c[1][6] = 0 (from 5); c[2][6] = 0 (the wait), c[2][7] = pen[2][7] + c[1][6] = 1.
    a2 = 3: the only origin of g in reach[2] is 7 (3, 9 and 13 are four steps from 5): total 1.
    a2 = 4: c[3][7] = pen[3][7] + min(c[2][7] = 1 (the wait), c[2][6] = 0 (from the left); 2, 8 and 12 are three steps
    from 5 and not in reach[2]) = 0, and 7 is again the only origin in reach[3]: total 0.  (0, 4) < (1, 3).
    Backtrack: 8 from 7 (the first move); 7 at layer 3: c[3][7] - pen = 0, the wait's c[2][7] = 1 is not it, from the left
    c[2][6] = 0 is: 6 at layer 2; 6 at layer 2: the wait's c[1][6] = 0 is it: 6 at layer 1; 6 at layer 1: 6 is not in
    reach[0], from the left 5 is."""
    s, (path, arrive, lb), pen = _focal(CROSSING, (3, 2))
    assert np.array_equal(pen, _crossing_penalty())
    assert path.tolist() == [5, 6, 6, 7, 8, 8, 8] and (arrive, lb) == (4, 3) and s.late == 1


def test_focal_route_at_w_1_may_not_wait():
    """w = 1: A = a = 3 and a2 = 3 is the only candidate, total 1: 8 from 7, 7 at layer 2 from 6 (7 is not in reach[1]),
    6 from 5: p itself, through the conflict on 7."""
    s, (path, arrive, lb), _ = _focal(CROSSING, (1, 1))
    assert path.tolist() == [5, 6, 7, 8, 8, 8, 8] and (arrive, lb) == (3, 3) and s.late == 0


def test_focal_route_takes_the_earlier_arrival_on_equal_totals():
    """The other robot comes down column 3 and is on g = 8 at layer 5 only: pen[v][8] = 1 for v = 4, 5, 6, so
    hold[3] = hold[4] = 3; its other cells 3 and 13 are on none of b's ways.  At w = 3/2 the candidates a2 = 3 and a2 = 4
    both have c = 0 before g: totals (3, 3) and (3, 4) tie on the total, and the earlier arrival is taken."""
    s, (path, arrive, lb), pen = _focal([3, 3, 3, 3, 3, 8, 13], (3, 2))
    assert pen[:, 1, 3].tolist() == [0, 0, 0, 0, 1, 1, 1]
    assert path.tolist() == [5, 6, 7, 8, 8, 8, 8] and (arrive, lb) == (3, 3)


# ---- the shared cases --------------------------------------------------------------------------------------------------
def test_every_shared_case_has_the_outcome_it_names(results):
    for name, r in results.items():
        assert r["outcome"] == CASES[name]["want"], (name, r["info"])
        assert len(r["info"]) == len(INFO) == 10
        if r["node"] >= 0:
            wn, wd = CASES[name]["w"]
            assert r["cost"] * wd <= wn * r["lb"] and r["bound"] <= r["lb"], (name, r["info"])
    # the search searches: at weight 1 only the one-robot case ends at the root
    assert [n for n, r in results.items() if r["expanded"] == 0 and n.endswith("@1_1")] == ["B1@1_1"]


def test_some_focal_route_arrives_later_than_it_could(results):
    """the late-arrival branch: at 3/2 the bay's robots are routed behind each other at the root already"""
    r = results["bay@3_2"]
    assert r["late"] >= 1 and r["arrive"].sum() > r["lb"]
    assert sum(r["late"] > 0 for r in results.values()) >= 10
    assert all(r["late"] == 0 for n, r in results.items() if n.endswith("@1_1"))


def test_property_e_weight_1_proves_the_cost_of_cbs(results):
    solved = 0
    for name, c in CBS_CASES.items():
        r, base = results[key(name, (1, 1))], run_cbs(c)
        if r["outcome"] == SOLVED and base["outcome"] == SOLVED:
            assert r["cost"] == r["bound"] == r["lb"] == base["cost"], (name, r["info"], base["info"])
            solved += 1
    assert solved >= 12


def test_properties_a_and_e_against_the_joint_optimum(small):
    searched = 0
    for c, best in small:
        for w in WEIGHTS:
            r = run(c, w=w)
            assert r["outcome"] == SOLVED, (w, r["info"])
            assert r["bound"] <= best <= r["cost"] and r["cost"] * w[1] <= w[0] * r["bound"], (w, best, r["info"])
            if w == (1, 1):
                assert r["cost"] == best
                searched += r["expanded"] > 0
    assert len(small) == 48 and searched >= 30


@pytest.mark.parametrize("E", [1, 2, 8])
@pytest.mark.parametrize("name", ["bay@21_20", "7x5_B3@1_1", "12x12_B4@21_20", "4x130@3_2"])
def test_property_b_the_bound_never_falls_and_slices_are_the_single_call(name, E):
    c = dict(CASES[name], expand=E)
    whole = run(c)
    n = whole["rounds_run"] + 1
    assert whole["outcome"] == SOLVED
    if n <= 20:
        bounds = [run(c, slices=[1] * k)["bound"] for k in range(1, n + 1)]
        assert bounds == sorted(bounds) and bounds[-1] == whole["bound"]
    for slices in ([n // 2, n - n // 2], [0, n], [n // 3, n // 3, n - 2 * (n // 3)]):
        part = run(c, slices=slices)
        for k in OUT:
            assert np.array_equal(part[k], whole[k]), (k, slices)


@pytest.mark.parametrize("base", ["7x5_B3", "12x12_B4", "skipped"])
def test_property_c_no_prioritised_plan_beats_the_bound(base, results):
    c = CBS_CASES[base]
    goal_cells, gi = problem(c)
    fields = fields_for(c["grid"], goal_cells, c["movement"])
    orders = list(itertools.permutations(range(len(c["starts"]))))[:24]
    p = plan_ref(c["grid"], c["starts"], gi, fields, goal_cells, orders, c["T"], c["sep2"], c["lag"], c["movement"])
    sums = [int(p["arrive"][g].sum()) for g in range(len(orders)) if np.all(p["status"][g] <= 0)]
    assert sums, "no failure-free order to hold against the bound"
    for w in WEIGHTS:
        r = results[key(base, w)]
        assert min(sums) >= r["bound"]
        for k in range(r["rounds_run"] + 1):                   # and against the bound of every slice on the way
            assert min(sums) >= run(CASES[key(base, w)], rounds=k)["bound"]


def test_property_d_a_conflict_free_node_meets_the_plans_guarantee(results):
    free = 0
    for name, r in results.items():
        c = CASES[name]
        if r["node"] < 0:
            continue
        bad = [q for q in conflicts(r["paths"], r["status"], c["grid"].shape[1], c["sep2"], c["lag"]) if q[2:] != (0, 0)]
        assert (bad == []) == bool(r["conflict_free"]), (name, bad)
        assert len(bad) == r["nconf"], (name, bad, r["nconf"])
        free += r["conflict_free"]
    assert free >= 40


def test_the_conflict_count_keeps_the_least_key_of_cbs(results):
    for name in ("bay", "12x12_B4", "skipped", "close_starts"):
        c = CBS_CASES[name]
        goal_cells, gi = problem(c)
        fields = fields_for(c["grid"], goal_cells, c["movement"])
        a = (c["grid"], c["starts"], gi, fields, goal_cells, c["T"], c["sep2"], c["lag"], c["movement"])
        root = cbs_ref(*a, rounds=0)["paths"]
        s = EcbsSearch(*a)
        assert s.conflict_count(root)[0] == CbsSearch.conflict(s, root) is not None


def test_the_stops_short_of_a_solution(results):
    pool, rounds = results["pool@1_1"], results["rounds@1_1"]
    # 9 expansions fit 20 ids; the incumbent of cost 18 is not yet within w of Lo = 16; a resumed call stops again
    assert pool["info"].tolist() == [POOL, 17, 1, 18, 16, 19, 9, 9, 18, 0]
    again = run(CASES["pool@1_1"], slices=[4096, 4096])
    for k in OUT:
        assert np.array_equal(again[k], pool[k])
    assert rounds["info"].tolist() == [ROUNDS, 5, 0, 16, 16, 15, 7, 7, 16, 1]
    assert run(CASES["pool@1_1"], nodes=1)["info"][:8].tolist() == [POOL, 0, 0, 12, 12, 1, 0, 0]
    assert results["infeasible@2_1"]["info"].tolist() == [INFEASIBLE, -1, 0, INF, INF, 2, 2, 2, INF, 0]
    # a dead root: robot 0 stands on an occupied cell that is walled in
    g = np.zeros((3, 3))
    g[0, 0] = g[0, 1] = g[1, 0] = g[1, 1] = 1.0
    dead = run(dict(HAND["bay"], grid=g, starts=[0, 8], goals=[8, 2], T=3, w=(3, 2)))
    assert dead["info"].tolist() == [INFEASIBLE, -1, 0, INF, INF, 0, 0, 0, INF, 0]


def test_the_case_with_many_nodes_needs_a_second_pass_of_the_selection():
    r = run(MANY)
    assert r["outcome"] == SOLVED and r["created"] > 1024 and r["repasses"] >= 1, (r["info"], r["repasses"])
    assert r["cost"] == r["bound"] == r["lb"] and r["conflict_free"] == 1


def test_the_store_with_four_robots_is_solved_within_its_budget():
    k = STORE4
    raw, g, starts, goals = store_case(k["B"], k["seed"], k["sep2"])
    c = dict(grid=g, starts=starts, goals=goals)
    goal_cells, gi = problem(c)
    fields = fields_for(g, goal_cells, k["movement"])
    r = ecbs_ref(g, starts, gi, fields, goal_cells, k["T"], k["sep2"], k["lag"], k["movement"], nodes=k["nodes"],
                 expand=k["expand"], rounds=k["rounds"], w=k["w"])
    print(r["info"].tolist(), "late", r["late"], "of", r["routes"])
    assert r["outcome"] == SOLVED and r["conflict_free"] == 1 and r["expanded"] == k["expansions"]
    assert r["cost"] * k["w"][1] <= k["w"][0] * r["bound"] and r["late"] >= 1
    assert conflicts(r["paths"], r["status"], g.shape[1], k["sep2"], k["lag"]) == []


# ---- the header and the binding ------------------------------------------------------------------------------------------
def test_symbols_are_declared_by_the_new_header_and_exported(lib):
    from robot_mpcs_amd import _abi
    assert lib.ECBS_SYMBOLS == SYMBOLS == list(_abi.ecbs_prototypes)
    check_header(lib, "rmpc_ecbs", SYMBOLS, _abi.ecbs_prototypes)
    vp, i = C.c_void_p, C.c_int
    S = _abi.ecbs_structs["rmpc_ecbs"]
    assert _abi.ecbs_prototypes[SYMBOLS[0]] == (C.c_int64, [i] * 6)
    assert _abi.ecbs_prototypes[SYMBOLS[1]] == (i, [C.POINTER(S), vp])
    assert _abi.ecbs_constants == {"RMPC_ECBS_MAX_W_DEN": 1024, "RMPC_ECBS_MAX_W": 4, "RMPC_ECBS_INFO": 10,
                                   "RMPC_ECBS_LB": 8, "RMPC_ECBS_NCONF": 9}
    assert [n.lower() for n in lib.ECBS_INFO_NAMES] == list(INFO) and lib.ECBS_INFO == len(INFO)
    # rmpc_cbs's members in their places, then the weight
    cbs = _abi.cbs_structs["rmpc_cbs"]
    assert S._fields_ == cbs._fields_ + [("w_num", C.c_int32), ("w_den", C.c_int32)]
    assert all(getattr(S, n).offset == getattr(cbs, n).offset for n, _ in cbs._fields_)
    assert list(_abi.ecbs_structs) == ["rmpc_ecbs"] and C.sizeof(S) == 160
    assert not set(SYMBOLS) & (set(_abi.prototypes) | set(_abi.cbs_prototypes)) and len(lib.CBS_SYMBOLS) == 2


def test_sizes(lib):
    L = lib.load_library()
    words = lambda H, W, T: 2 * (T + 1) * H * ((W + 63) // 64) + 2 * H * ((W + 63) // 64) + (H * W + 1) // 2
    for H, W, T, B, M, E in ((7, 5, 9, 3, 64, 1), (65, 70, 70, 3, 4096, 8), (128, 128, 1023, 64, 1 << 20, 256),
                             (1, 1, 1, 1, 1, 1), (41, 41, 128, 16, 4096, 16)):
        # a slot: the planner's parts and the int32 path, a byte per (t, cell), three int32 rows of cells
        slot = words(H, W, T) + (T + 2) // 2 + ((T + 1) * H * W + 7) // 8 + (3 * H * W + 1) // 2
        want = 8 * 4 + 4 * 256 + 8 * H * ((W + 63) // 64) + 8 * M + 8 * slot * 2 * E + 24 * M + 4 * M * B + 2 * M * B * (T + 1)
        assert lib.ecbs_work_bytes(H, W, T, B, M, E) == (want + 7) // 8 * 8
        assert lib.ecbs_work_bytes(H, W, T, B, M, E) > lib.cbs_work_bytes(H, W, T, B, M, E)
    for a in ((0, 5, 9, 3, 64, 1), (129, 128, 9, 3, 64, 1), (7, 5, 0, 3, 64, 1), (7, 5, 1024, 3, 64, 1), (7, 5, 9, 0, 64, 1),
              (7, 5, 9, 65, 64, 1), (7, 5, 9, 3, 0, 1), (7, 5, 9, 3, (1 << 20) + 1, 1), (7, 5, 9, 3, 64, 0), (7, 5, 9, 3, 64, 257)):
        assert L.rmpc_ecbs_work_bytes(*a) == -1 and L.rmpc_last_error().decode().startswith("ecbs: need")
        with pytest.raises(lib.RmpcError, match="ecbs: need"):
            lib.ecbs_work_bytes(*a)


ARGS = dict(H=7, W=5, movement=4, grid=P_, occ_threshold=0.8, B=3, Gf=2, start_cell=P_, goal_index=P_, fields=P_,
            goal_cells=P_, T=9, sep2=2, lag=1, nodes=64, expand=2, rounds=4, resume=0, work=P_, work_bytes=1 << 22, paths=P_,
            status=P_, arrive=P_, info=P_, w_num=11, w_den=10)
REFUSALS = [(dict([(k, None)]), NULL) for k, v in ARGS.items() if v == P_]
REFUSALS += [(dict(B=0), "ecbs: need 1 <= B <= RMPC_CBS_MAX_ROBOTS = 64"), (dict(B=65), "ecbs: need 1 <= B"),
             (dict(T=0), "ecbs: need 1 <= T"), (dict(T=1024), "ecbs: need 1 <= T <= RMPC_TIMED_MAX_T = 1023"),
             (dict(sep2=0), "ecbs: need 1 <= sep2"), (dict(sep2=4097), "ecbs: need 1 <= sep2"),
             (dict(lag=0), "ecbs: lag must lie"), (dict(lag=5), "ecbs: lag must lie"),
             (dict(nodes=0), "ecbs: need 1 <= nodes <= RMPC_CBS_MAX_NODES = 1048576"), (dict(nodes=(1 << 20) + 1), "ecbs: need 1 <= nodes"),
             (dict(expand=0), "ecbs: need 1 <= expand <= RMPC_CBS_MAX_EXPAND = 256"), (dict(expand=257), "ecbs: need 1 <= expand"),
             (dict(rounds=-1), "ecbs: need 0 <= rounds <= RMPC_CBS_MAX_ROUNDS = 4096"), (dict(rounds=4097), "ecbs: need 0 <= rounds"),
             (dict(rounds=I_MAX), "ecbs: need 0 <= rounds"),
             (dict(w_den=0), "ecbs: need 1 <= w_den <= RMPC_ECBS_MAX_W_DEN = 1024"), (dict(w_den=-1), "ecbs: need 1 <= w_den"),
             (dict(w_num=1025, w_den=1025), "ecbs: need 1 <= w_den"),
             (dict(w_num=9, w_den=10), "ecbs: need w_den <= w_num <= RMPC_ECBS_MAX_W * w_den, RMPC_ECBS_MAX_W = 4"),
             (dict(w_num=0, w_den=1), "ecbs: need w_den <= w_num"), (dict(w_num=41, w_den=10), "ecbs: need w_den <= w_num"),
             (dict(w_num=I_MAX, w_den=1024), "ecbs: need w_den <= w_num"),
             (dict(movement=6), "grid: movement"), (dict(H=0), "grid: need"), (dict(W=0), "grid: need"),
             (dict(H=129, W=128), "ecbs: need H, W >= 1 and H*W <="), (dict(Gf=0), "ecbs: need 1 <= G"), (dict(Gf=I_MAX), "ecbs: need 1 <= G"),
             (dict(struct_size=152), "rmpc_ecbs.struct_size mismatch"), (dict(struct_size=0), "rmpc_ecbs.struct_size mismatch"),
             (dict(work_bytes=0), "ecbs: the workspace holds 0 bytes"), (dict(work_bytes=-1), "ecbs: the workspace holds -1 bytes")]


@pytest.mark.parametrize("bad,want", REFUSALS, ids=[",".join("%s=%s" % kv for kv in b.items()) for b, _ in REFUSALS])
def test_the_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    L = lib.load_library()
    a = filled(lib.EcbsArgs, ARGS, **bad)
    refused(L, L.rmpc_ecbs_device(C.byref(a), None), want)
    assert L.rmpc_ecbs_device(None, None) == -1 and L.rmpc_last_error().decode() == NULL


def test_a_workspace_one_byte_short_is_refused_also_when_resumed(lib):
    L = lib.load_library()
    for resume in (0, 1):
        a = filled(lib.EcbsArgs, ARGS, resume=resume, work_bytes=lib.ecbs_work_bytes(7, 5, 9, 3, 64, 2) - 1)
        assert L.rmpc_ecbs_device(C.byref(a), None) == -1
        assert "are needed (rmpc_ecbs_work_bytes)" in L.rmpc_last_error().decode()


def test_the_limit_weights_are_taken(lib):
    """w_den = 1024 and w_num = 4 w_den pass the weight's check: the call is refused only further on, for its workspace"""
    L = lib.load_library()
    a = filled(lib.EcbsArgs, ARGS, w_num=4096, w_den=1024, work_bytes=8)
    refused(L, L.rmpc_ecbs_device(C.byref(a), None), "ecbs: the workspace holds 8 bytes")
