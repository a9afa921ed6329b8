"""Traffic-aware routes (include/rmpc_traffic.h), what needs no GPU: the hand case of the swap; the
restatement against a plain heap Dijkstra; zero weights against the global planner's restatement; the best-response and
potential properties of ``plan`` with groups of one; the table invariant; the new header with its tables; every refusal
of the four entries."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import global_planner_reference as gp
from traffic_cases import COSTS, FLOWS, OCC, UNIT, field_map, flow_table, fleet_case, goal_list, swap_case
from traffic_reference import (INF, OK, add_ref, count_routes, descend_ref, empty_flow, field_heap, field_ref, make_costs, plan_ref,
                               refused, route_cost, score_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rmpc_grid_traffic_add_device", "rmpc_grid_fields_traffic_device", "rmpc_grid_paths_traffic_device",
           "rmpc_grid_traffic_score_device"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return _lib


# ---- the hand case ----------------------------------------------------------------------------------------------------
def test_swap_on_the_open_map_by_hand():
    """both robots first take the middle row: (L, V, C) = (12, 7, 6).  Robot 0's step moves it to row 2, down first
    (+row precedes -row in the move order): cells 7, 14 .. 20, 13.  Robot 1 keeps its route: (14, 2, 0)."""
    grid, starts, goals, k = swap_case()
    seen = []
    routes, lens, flow, scores = plan_ref(grid, OCC, k, starts, goals, movement=4, groups=2, rounds=1,
                                          on_step=lambda bs, old, new, others: seen.append((bs, old, new)))
    assert seen[0] == ([0], [list(range(7, 14))], [[7] + list(range(14, 21)) + [13]])
    assert seen[1] == ([1], [list(range(13, 6, -1))], [list(range(13, 6, -1))])
    assert scores.tolist() == [[12, 7, 6], [14, 2, 0]] and lens.tolist() == [9, 7]
    assert routes == [[7, 14, 15, 16, 17, 18, 19, 20, 13], [13, 12, 11, 10, 9, 8, 7]]
    assert np.array_equal(flow, count_routes(3, 7, routes))


def test_edge_cost_counts_the_routes_that_step_back_onto_the_cell():
    """one route 8 -> 9 -> 10 on the 3 x 7 map: stepping 10 -> 9 (move 2) meets the route's step 9 -> 10 (plane 0 at 9),
    stepping 9 -> 10 does not; a visited cell costs w_visit whichever way it is entered"""
    from traffic_reference import edge_cost
    flow = count_routes(3, 7, [[8, 9, 10]])
    assert flow[0].ravel()[[8, 9, 10]].tolist() == [1, 1, 0] and flow[8].ravel()[[8, 9, 10]].tolist() == [1, 1, 1]
    assert flow.sum() == 5
    k = make_costs(10, 14, 3, 4, 100, 5)
    assert edge_cost(flow, k, 10, 2, 7) == 10 + 3 + 100 and edge_cost(flow, k, 9, 0, 7) == 10 + 3
    assert edge_cost(flow, k, 2, 1, 7) == 10 + 3 and edge_cost(flow, k, 1, 4, 7) == 14 + 3 and edge_cost(flow, k, 0, 0, 7) == 10
    flow[8, 1, 2], flow[0, 1, 2] = 9, -3                              # above the cap; a negative entry counts as 0
    assert edge_cost(flow, k, 10, 2, 7) == 10 + 3 * 4 + 0


def test_add_skips_what_the_header_says_it_skips_and_remove_undoes_it():
    flow = flow_table("negative", 3, 7)
    before = flow.copy()
    paths = np.array([[0, 1, 1, 8, 20, 6], [7, 8, 9, 0, 0, 0], [6, 7, 21, -1, 3, 4], [1, 2, 3, 4, 5, 6]], np.int64)
    lens, select = np.array([6, 0, 9, 2]), np.array([1, 1, 5, 0])
    add_ref(flow, paths, lens, 1, select)
    d = flow - before
    # robot 0: 0 -> 1 a move, 1 == 1 nothing, 1 -> 8 a move, 8 -> 20 and 20 -> 6 not adjacent; robot 2: 6 -> 7 wraps the
    # row's end (no move), 21 and -1 are outside the map, 3 -> 4 a move; robots 1 (no route) and 3 (not selected) nothing
    assert d[8].ravel().tolist() == [1, 2, 0, 1, 1, 0, 2, 1, 1] + [0] * 11 + [1]
    assert d[0].ravel()[[0, 3]].tolist() == [1, 1] and d[1].ravel()[1] == 1 and d[:8].sum() == 3
    add_ref(flow, paths, lens, -1, select)
    assert np.array_equal(flow, before)


# ---- the two restatements ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("movement", [4, 8])
@pytest.mark.parametrize("kind", FLOWS)
@pytest.mark.parametrize("size", [(1, 37), (21, 21), (25, 41)])
def test_restatement_equals_the_heap_dijkstra(size, kind, movement):
    grid = field_map(*size)
    flow = flow_table(kind, *size)
    for goal in goal_list(grid, 6):
        a, sa = field_ref(grid, OCC, flow, COSTS, int(goal), movement)
        b, sb = field_heap(grid, OCC, flow, COSTS, int(goal), movement)
        assert sa == sb and a.dtype == np.int32 and np.array_equal(a, b)
        assert (a == INF).all() if sa != OK else a.flat[goal] == 0
        if sa == OK and size != (1, 37):                                # the walled box is free and apart from the rest
            inside = 3 <= goal // size[1] < 6 and 3 <= goal % size[1] < 6
            assert (a[3:6, 3:6] < INF).all() and (a < INF).sum() == 9 if inside else (a[3:6, 3:6] == INF).all() and (a < INF).sum() > 100


# ---- zero weights: the global planner's field and route -----------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_zero_weights_are_the_global_planners_values_and_routes(seed):
    grid, starts, goals = fleet_case(seed=seed)
    flow = flow_table("above", 21, 21, seed)                            # with zero weights the table does not matter
    for s, g in zip(starts[:8], goals[:8]):
        D, st = field_ref(grid, OCC, flow, UNIT, int(g), 4)
        want = gp.field_ref(grid, int(g), 4, 0.0, OCC)
        assert st == OK and np.array_equal(np.where(D == INF, np.inf, D.astype(np.float64)), want)
        cells, n = descend_ref(grid, OCC, flow, UNIT, D, int(s), int(g), 4)
        assert n == len(cells) > 1 and cells == gp.descend_ref(grid, want, int(s), int(g), 4, 0.0)


# ---- best response and potential ----------------------------------------------------------------------------------------
ROUNDS = 6          # the fleet of 24 is at rest after four rounds with 4 moves and after two with 8 (counted with this rule)


@pytest.mark.parametrize("movement", [4, 8])
def test_groups_of_one_are_a_best_response_and_the_potential_falls_by_the_saving(movement):
    grid, starts, goals = fleet_case()
    k, W = COSTS, grid.shape[1]
    routes = {}

    def potential(flow):
        L, V, Cf = score_ref(flow, k["base_axial"], k["base_diag"])
        return L + k["w_visit"] * V + k["w_contra"] * Cf

    def on_step(bs, old, new, others):
        (b,), (o,), (n,) = bs, old, new
        assert others.min() >= 0 and others[8].max() < k["cap_visit"] and others[:8].max() < k["cap_contra"]   # no cap binds
        saving = route_cost(others, k, o, W) - route_cost(others, k, n, W)
        assert saving >= 0                                              # the new route is a best response
        assert len(set(n)) == len(n) and n[0] == starts[b] and n[-1] == goals[b]
        routes[b] = n
        before = potential(others + count_routes(*grid.shape, [o]))
        after = potential(others + count_routes(*grid.shape, [n]))
        assert before - after == saving
        moved.append(o != n)

    moved = []
    out = plan_ref(grid, OCC, k, starts, goals, movement, groups=24, rounds=ROUNDS, on_step=on_step)
    final, lens, flow, scores = out
    assert (lens > 1).all() and len(moved) == ROUNDS * 24
    pot = [potential_of(s, k) for s in scores]
    assert all(a >= b for a, b in zip(pot[:-1], pot[1:])) and pot[0] > pot[-1]
    assert flow[8].max() < k["cap_visit"] and flow[:8].max() < k["cap_contra"]
    # a round in which nobody moved repeats for ever: the state a round starts from is the one it left
    rounds = [moved[24 * r:24 * r + 24] for r in range(ROUNDS)]
    quiet = [r for r in range(ROUNDS) if not any(rounds[r])]
    assert quiet, "no equilibrium within %d rounds" % ROUNDS
    assert all(not any(rounds[r]) for r in  range(quiet[0], ROUNDS))
    assert all((scores[r + 1] == scores[quiet[0] + 1]).all() for r in  range(quiet[0], ROUNDS))


def potential_of(score, k):
    return int(score[0]) + k["w_visit"] * int(score[1]) + k["w_contra"] * int(score[2])


# ---- the table invariant ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 5, 24])
def test_table_after_plan_is_a_recount_of_the_final_routes(groups):
    grid, starts, goals = fleet_case()
    routes, lens, flow, scores = plan_ref(grid, OCC, COSTS, starts, goals, 8, groups=groups, rounds=2)
    assert np.array_equal(flow, count_routes(*grid.shape, routes)) and flow.dtype == np.int32
    assert scores.shape == (3, 3) and tuple(scores[-1]) == score_ref(flow, COSTS["base_axial"], COSTS["base_diag"])
    assert flow[8].sum() == lens.sum() and flow[:8].sum() == (lens - 1).sum()


# ---- the header and the binding ---------------------------------------------------------------------------------------
def test_traffic_symbols_are_declared_by_the_new_header_and_exported(lib):
    """the test that fails on the parent: the header, its tables and the four entries are new"""
    from robot_mpcs_amd import _abi
    assert lib.TRAFFIC_SYMBOLS == SYMBOLS == list(_abi.traffic_prototypes)
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rmpc_traffic.h")).read(), flags=re.S)
    code = re.sub(r"^[ \t]*#.*$", "", code, flags=re.M)
    assert sorted(set(re.findall(r"\b(rmpc_\w+)\s*\(", code))) == sorted(SYMBOLS)
    L = lib.load_library()
    for sym in SYMBOLS:
        fn = getattr(L, sym)
        assert (fn.restype, list(fn.argtypes)) == (_abi.traffic_prototypes[sym][0], _abi.traffic_prototypes[sym][1])
    vp, i, d, k = C.c_void_p, C.c_int, C.c_double, C.POINTER(lib.TrafficCostsArgs)
    assert _abi.traffic_prototypes[SYMBOLS[0]] == (i, [i, i, i, vp, vp, i, vp, i, vp, vp])
    assert _abi.traffic_prototypes[SYMBOLS[1]] == (i, [i, i, vp, d, vp, k, i, vp, i, vp, vp, vp, vp])
    assert _abi.traffic_prototypes[SYMBOLS[2]] == (i, [i, i, vp, d, vp, k, i, vp, vp, i, vp, vp, i, i, vp, vp, vp])
    assert _abi.traffic_prototypes[SYMBOLS[3]] == (i, [i, i, vp, i, i, vp, vp])
    assert _abi.traffic_constants == {"RMPC_TRAFFIC_PLANES": 9, "RMPC_TRAFFIC_MAX_EDGE": 65535, "RMPC_TRAFFIC_MAX_CAP_VISIT": 255,
                                      "RMPC_TRAFFIC_MAX_CAP_CONTRA": 15, "RMPC_TRAFFIC_INF": INF}
    assert [f[0] for f in lib.TrafficCostsArgs._fields_] == ["struct_size", "base_axial", "base_diag", "w_visit", "cap_visit",
                                                             "w_contra", "cap_contra"] and C.sizeof(lib.TrafficCostsArgs) == 28
    c = lib.traffic_costs()
    assert (c.struct_size, c.base_axial, c.base_diag, c.w_visit, c.cap_visit, c.w_contra, c.cap_contra) == (28, *COSTS.values())
    # rmpc.h declares what it declared
    assert len(lib.EXPORTED_SYMBOLS) == 65 and _abi.constants["RMPC_VERSION"] == 201
    assert not set(SYMBOLS) & set(_abi.prototypes)
    with open(os.path.join(ROOT, "robot_mpcs_amd", "csrc", "sources.txt")) as f:
        listed = f.read().split()
    assert "include/rmpc_traffic.h" in listed and "robot_mpcs_amd/csrc/rmpc_traffic.hpp" in listed
    from robot_mpcs_amd import global_planner
    from robot_mpcs_amd.global_planner.traffic import TrafficRoutes
    assert global_planner.TrafficRoutes is TrafficRoutes and callable(TrafficRoutes.plan) and callable(TrafficRoutes.replan)


# ---- the refusals: before any HIP call, so without a GPU ------------------------------------------------------------------
P_ = 0x1000      # a host-side fake pointer: a refusal never dereferences it
I_MAX = 2 ** 31 - 1
NULL = "null argument"
HW = ": need H, W >= 1"


def too_large(H, W):
    return ": %dx%d map exceeds RMPC_GRID_MAX_CELLS = 16384 cells" % (H, W)


MAP_REFUSALS = [(dict(H=0), HW), (dict(W=0), HW), (dict(H=-3), HW), (dict(H=129, W=128), too_large(129, 128)),
                (dict(H=I_MAX, W=I_MAX), too_large(I_MAX, I_MAX))]
MOVEMENT = [(dict(movement=v), ": movement must be 4 or 8") for v in (0, 5, 9, -4)]
BASE = ": base_axial and base_diag must be >= 1"
NEG = ": weights and caps must be >= 0"
EDGE = ": the largest edge cost %d exceeds RMPC_TRAFFIC_MAX_EDGE = 65535"
COST_REFUSALS = [(dict(struct_size=24), "rmpc_traffic_costs.struct_size mismatch"), (dict(base_axial=0), BASE), (dict(base_diag=0), BASE),
                 (dict(base_axial=-1000), BASE), (dict(w_visit=-1), NEG), (dict(w_contra=-1), NEG), (dict(cap_visit=-1), NEG),
                 (dict(cap_contra=-1), NEG), (dict(cap_visit=256), ": cap_visit exceeds RMPC_TRAFFIC_MAX_CAP_VISIT = 255"),
                 (dict(cap_contra=16), ": cap_contra exceeds RMPC_TRAFFIC_MAX_CAP_CONTRA = 15"),
                 (dict(base_diag=65536), EDGE % (65536 + 300 * 32 + 700 * 15)), (dict(w_visit=1720), EDGE % (1414 + 1720 * 32 + 700 * 15)),
                 (dict(w_contra=I_MAX, w_visit=I_MAX, cap_visit=255), EDGE % (1414 + I_MAX * 255 + I_MAX * 15))]


def refusals(who, cases):
    ids = [",".join("%s=%s" % kv for kv in bad.items()) for bad, _ in cases]
    exact = (NULL, "rmpc_traffic_costs.struct_size mismatch")
    return pytest.mark.parametrize("bad,want", [(b, w if w in exact else who + w) for b, w in cases], ids=ids)


def call(lib, name, args, bad):
    """the entry with ``bad`` put over ``args``; the members of the costs are taken out of ``bad`` into the struct"""
    L = lib.load_library()
    costs = lib.traffic_costs()
    for f, v in bad.items():
        if hasattr(costs, f):
            setattr(costs, f, v)
    a = dict(args, **{f: v for f, v in bad.items() if not hasattr(costs, f)})
    assert set(a) == set(args)
    if a.get("costs") == "costs":
        a["costs"] = C.byref(costs)
    return getattr(L, name)(*a.values()), L.rmpc_last_error().decode()


def test_the_largest_edge_cost_at_the_limit_is_accepted_by_the_rule():
    assert not refused(make_costs()) and not refused(make_costs(65535, 1, 0, 0, 0, 0)) and refused(make_costs(65536, 1, 0, 0, 0, 0))
    assert not refused(make_costs(1000, 1414, 251, 255, 7, 15)) and refused(make_costs(1000, 1414, 252, 255, 7, 15))
    for bad, _ in COST_REFUSALS[1:]:
        assert refused(dict(COSTS, **bad)), bad


ADD = dict(H=41, W=41, B=24, path=P_, len=P_, max_len=164, select=None, sign=1, flow=P_, stream=None)
SIZES = ": need B, max_len >= 1 and B*max_len <= INT_MAX"
ADD_REFUSALS = [(dict([(k, None)]), NULL) for k in ("path", "len", "flow")] + MAP_REFUSALS
ADD_REFUSALS += [(dict(B=0), SIZES), (dict(max_len=0), SIZES), (dict(B=-1), SIZES), (dict(B=1 << 16, max_len=1 << 15), SIZES)]
ADD_REFUSALS += [(dict(sign=v), ": sign must be +1 or -1") for v in (0, 2, -2, I_MAX)]


@refusals("grid traffic add", ADD_REFUSALS)
def test_add_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    assert call(lib, "rmpc_grid_traffic_add_device", ADD, bad) == (-1, want)


FIELDS = dict(H=41, W=41, grid=P_, occ=0.8, flow=P_, costs="costs", G=3, goals=P_, movement=8, fields=P_, status=P_, sweeps=None,
              stream=None)
GS = ": need 1 <= G and G*H*W <= INT_MAX"
FIELDS_REFUSALS = [(dict([(k, None)]), NULL) for k in ("grid", "flow", "costs", "goals", "fields", "status")] + MAP_REFUSALS + MOVEMENT
FIELDS_REFUSALS += [(dict(G=0), GS), (dict(G=-2), GS), (dict(G=I_MAX), GS), (dict(occ=float("nan")), ": occ_threshold must not be a NaN")]
FIELDS_REFUSALS += COST_REFUSALS


@refusals("grid fields traffic", FIELDS_REFUSALS)
def test_fields_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    assert call(lib, "rmpc_grid_fields_traffic_device", FIELDS, bad) == (-1, want)


PATHS = dict(H=41, W=41, grid=P_, occ=0.8, flow=P_, costs="costs", G=3, fields=P_, goals=P_, B=24, start=P_, index=P_, movement=8,
             max_len=164, path=P_, len=P_, stream=None)
PATHS_REFUSALS = [(dict([(k, None)]), NULL) for k in ("grid", "flow", "costs", "fields", "goals", "start", "index", "path", "len")]
PATHS_REFUSALS += MAP_REFUSALS + MOVEMENT + [(dict(G=0), GS), (dict(B=0), SIZES), (dict(max_len=0), SIZES), (dict(max_len=-1), SIZES),
                                             (dict(B=1 << 16, max_len=1 << 15), SIZES),
                                             (dict(occ=float("nan")), ": occ_threshold must not be a NaN")] + COST_REFUSALS


@refusals("grid paths traffic", PATHS_REFUSALS)
def test_paths_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    assert call(lib, "rmpc_grid_paths_traffic_device", PATHS, bad) == (-1, want)


SCORE = dict(H=41, W=41, flow=P_, base_axial=1000, base_diag=1414, score=P_, stream=None)
SCORE_REFUSALS = [(dict([(k, None)]), NULL) for k in ("flow", "score")] + MAP_REFUSALS
SCORE_REFUSALS += [(dict(base_axial=0), BASE), (dict(base_diag=0), BASE), (dict(base_diag=-5), BASE)]


@refusals("grid traffic score", SCORE_REFUSALS)
def test_score_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    L = lib.load_library()
    assert set(bad) <= set(SCORE)
    assert L.rmpc_grid_traffic_score_device(*dict(SCORE, **bad).values()) == -1
    assert L.rmpc_last_error().decode() == want


def test_wrappers_and_class_refuse_mismatched_arguments(lib):
    import torch
    from robot_mpcs_amd.global_planner import TrafficRoutes
    i32 = dict(dtype=torch.int32)
    flow, grid = torch.zeros((9, 4, 6), **i32), torch.zeros((4, 6), dtype=torch.float64)
    path, lens = torch.zeros((3, 8), **i32), torch.zeros(3, **i32)
    for f in (torch.zeros((8, 4, 6), **i32), torch.zeros((9, 4, 6), dtype=torch.int64), torch.zeros((9, 6, 4), **i32).transpose(1, 2)):
        with pytest.raises(ValueError, match="grid_traffic_add_device"):
            lib.grid_traffic_add_device(f, path, lens)
        with pytest.raises(ValueError, match="grid_traffic_score_device"):
            lib.grid_traffic_score_device(f, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="grid_traffic_add_device"):
        lib.grid_traffic_add_device(flow, path, lens[:2])
    with pytest.raises(ValueError, match="grid_traffic_add_device"):
        lib.grid_traffic_add_device(flow, path, lens, select=torch.zeros(4, **i32))
    with pytest.raises(ValueError, match="grid_traffic_score_device"):
        lib.grid_traffic_score_device(flow, torch.zeros(3, **i32))
    goals, status = torch.zeros(2, **i32), torch.zeros(2, **i32)
    for fields in (torch.zeros((3, 4, 6), **i32), torch.zeros((2, 4, 6), dtype=torch.float64), torch.zeros((2, 6, 4), **i32)):
        with pytest.raises(ValueError, match="grid_fields_traffic_device"):
            lib.grid_fields_traffic_device(grid, flow, lib.traffic_costs(), goals, fields, status)
    with pytest.raises(ValueError, match="grid_paths_traffic_device"):
        lib.grid_paths_traffic_device(grid, flow, lib.traffic_costs(), torch.zeros((1, 4, 6), **i32), goals, lens, lens, path, lens)
    with pytest.raises(ValueError, match="grid_paths_traffic_device"):
        lib.grid_paths_traffic_device(grid, flow, lib.traffic_costs(), torch.zeros((2, 4, 6), **i32), goals, lens, lens, path[:2], lens)
    for kw in (dict(groups=0), dict(groups=4), dict(rounds=-1), dict(movement="6N"), dict(starts=[0, 1]),
               dict(grid=np.zeros((129, 128)))):
        a = dict(dict(grid=np.zeros((4, 6)), starts=[0, 1, 2], goal_cells=[5, 6, 7], device="cpu"), **kw)
        with pytest.raises(ValueError, match="TrafficRoutes|movement"):
            TrafficRoutes(**a)
