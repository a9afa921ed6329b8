"""The minimum-cost assignment (include/rmpc_assign_opt.h), what needs no GPU: the restatement
(tests/assign_optimal_reference.py) on hand-worked cases and against scipy's optimum, the header's bounds on Python
integers, the third header and its tables, and every refusal of the two entries."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from assign_optimal_cases import KINDS, make_costs
from assign_optimal_reference import MAX_Q, assign_optimal_ref, check_matching, oriented, quantise, sap, sap_python

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = math.inf, math.nan
SYMBOLS = ["rmpc_assign_optimal_work_bytes", "rmpc_assign_optimal_device"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return _lib


# ---- the restatement on cases worked by hand --------------------------------------------------------------------------
def test_quantisation_rounds_half_to_even_and_knows_the_takeable_pairs():
    c = np.array([[0.5, 1.5, 2.5, -0.0, NAN, -1e-9, INF, -INF], [2.0 ** 20, 2.0 ** 20 + 0.5, 2.0 ** 20 + 0.51, 1e308, 0.49, 3.0, 0.0, 1.0]])
    assert quantise(c, 1.0).tolist() == [[0, 2, 2, 0, -1, -1, -1, -1], [MAX_Q, MAX_Q, -1, -1, 0, 3, 0, 1]]
    assert quantise(np.array([[1.0, 0.3, 1e-4]]), 1024.0).tolist() == [[1024, 307, 0]]
    assert quantise(np.array([[1e308]]), 1e10).tolist() == [[-1]]          # the product overflows to +inf


def test_two_by_two_with_a_tie_takes_the_lowest_columns():
    a, total, count, steps = assign_optimal_ref(np.ones((2, 2)), 1.0)
    assert a.tolist() == [0, 1] and (total, count, steps) == (2, 2, 3)


def test_two_by_two_where_the_second_row_moves_the_first():
    """row 1 takes column 1; row 2 finds it there (delta 1), looks on through row 1 at column 2 (2 - 1 = 1) and swaps"""
    a, total, count, steps = assign_optimal_ref(np.array([[1.0, 2.0], [1.0, 5.0]]), 1.0)
    assert a.tolist() == [1, 0] and (total, count, steps) == (3, 2, 3)
    C_, P, by_robot = oriented(quantise(np.array([[1.0, 2.0], [1.0, 5.0]]), 1.0))
    assert by_robot and P == 2 * 5 + 1 and sap(C_)[0].tolist()[1:] == [2, 1]


def test_three_by_two_is_solved_with_the_targets_as_rows():
    """B > T: target 0 sees (4, 1, 3) and takes robot 1, target 1 sees (P, 2, 1) and takes robot 2; robot 0 stays"""
    cost = np.array([[4.0, INF], [1.0, 2.0], [3.0, 1.0]])
    C_, P, by_robot = oriented(quantise(cost, 1.0))
    assert not by_robot and P == 2 * 4 + 1 and C_.tolist() == [[4, 1, 3], [9, 2, 1]]
    a, total, count, steps = assign_optimal_ref(cost, 1.0)
    assert a.tolist() == [-1, 0, 1] and (total, count, steps) == (2, 2, 2)


def test_two_by_three_with_a_robot_nobody_may_take():
    """robot 0 has no takeable pair: its row is all P = 2 * 2 + 1, it holds column 1 and is reported as -1"""
    cost = np.array([[NAN, -1.0, INF], [2.0, 0.0, 1.0]])
    a, total, count, steps = assign_optimal_ref(cost, 1.0)
    assert a.tolist() == [-1, 1] and (total, count, steps) == (0, 1, 2)
    # with the hole elsewhere the robots share out the columns: 0 + 1 beats 2 + ...
    a, total, count, steps = assign_optimal_ref(np.array([[0.0, INF, 5.0], [2.0, 0.0, 1.0]]), 1.0)
    assert a.tolist() == [0, 1] and (total, count) == (0, 2)


def test_all_untakeable():
    a, total, count, steps = assign_optimal_ref(np.full((3, 2), NAN))
    assert a.tolist() == [-1, -1, -1] and (total, count) == (0, 0)


def test_python_integer_loop_is_the_numpy_loop():
    for kind in KINDS:
        for B, T in ((3, 5), (5, 3), (17, 13)):
            C_, _, _ = oriented(quantise(make_costs(kind, B, T, holes=True)))
            p, steps = sap(C_)
            pp, psteps, _ = sap_python(C_.tolist())
            assert p.tolist()[1:] == pp[1:] and steps == psteps


# ---- against scipy's optimum ------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (3, 5), (5, 3), (65, 63), (130, 17), (17, 130), (257, 255)]
CASES = [(k, h, B, T) for k in KINDS for h in (False, True) for B, T in SHAPES]
CASES += [(k, False, 1024, 1024) for k in ("unif", "grid")]


@pytest.mark.parametrize("kind,holes,B,T", CASES, ids=["%s%s-%dx%d" % (k, "-holes" if h else "", B, T) for k, h, B, T in CASES])
def test_restatement_reaches_scipys_optimum(kind, holes, B, T):
    """a valid matching on takeable pairs whose pair count and sum of q are those of linear_sum_assignment on the same
    integer matrix with P substituted: its optimum k P + s splits uniquely, since s <= m Qmax < P"""
    from scipy.optimize import linear_sum_assignment
    cost = make_costs(kind, B, T, holes)
    q = quantise(cost)
    a, total, count, steps = assign_optimal_ref(cost)
    assert check_matching(q, a) == (count, total)
    C_, P, _ = oriented(q)
    m = C_.shape[0]
    r, c = linear_sum_assignment(C_)
    best = int(C_[r, c].sum())
    assert (m - count) * P + total == best and total < P
    assert steps >= m
    if holes and min(B, T) > 1:
        assert count < m                              # the row and the column nobody may take


# ---- the header's bounds ----------------------------------------------------------------------------------------------
def test_bounds_of_the_header_on_its_worst_case():
    """0 <= u <= Cmax, -Cmax <= v <= 0, 0 <= minv <= 2 Cmax and the key below 2^45, reached on the matrix the header
    names with Cmax = 2^30 + 1 = the greatest P; never exceeded on matrices of 0 and Cmax or of random values"""
    K = 1024 * MAX_Q + 1
    assert K == 2 ** 30 + 1
    p, steps, ext = sap_python([[0, K, K], [0, K, K], [K, K, K]])
    assert ext == dict(u_max=K, v_min=-K, minv_max=2 * K, key_max=((2 * K) << 13) | 1)
    assert ext["key_max"] < 2 ** 45 and 2 * K == 2 ** 31 + 2
    rng = np.random.default_rng(3)
    for trial in range(60):
        m = int(rng.integers(1, 9))
        n = m + int(rng.integers(0, 4))
        M = rng.integers(0, 2, size=(m, n)) * K if trial % 2 else rng.integers(0, K + 1, size=(m, n))
        _, _, ext = sap_python(M.tolist())
        assert ext["u_max"] <= K and ext["v_min"] >= -K and ext["minv_max"] <= 2 * K and ext["key_max"] < 2 ** 45


# ---- the header and the binding ---------------------------------------------------------------------------------------
def test_assign_symbols_are_declared_by_the_new_header_and_exported(lib):
    from robot_mpcs_amd import _abi
    assert lib.ASSIGN_OPT_SYMBOLS == SYMBOLS == list(_abi.assign_prototypes)
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rmpc_assign_opt.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(rmpc_\w+)\s*\(", code))) == sorted(SYMBOLS)
    L = lib.load_library()
    for sym in SYMBOLS:
        fn = getattr(L, sym)
        assert (fn.restype, list(fn.argtypes)) == (_abi.assign_prototypes[sym][0], _abi.assign_prototypes[sym][1])
    vp = C.c_void_p
    assert _abi.assign_prototypes[SYMBOLS[0]] == (C.c_int64, [C.c_int] * 3)
    assert _abi.assign_prototypes[SYMBOLS[1]] == (C.c_int, [C.c_int] * 3 + [vp, C.c_double] + [vp] * 5 + [C.c_int64, vp])
    assert _abi.assign_constants == {"RMPC_ASSIGN_OPT_MAX_Q": 1 << 20} and lib.ASSIGN_OPT_MAX_Q == MAX_Q == 1 << 20
    # rmpc.h and rmpc_grid_large.h declare what they declared
    assert len(lib.EXPORTED_SYMBOLS) == 65 and len(lib.GRID_LARGE_SYMBOLS) == 2
    assert not set(SYMBOLS) & (set(_abi.prototypes) | set(_abi.large_prototypes))
    with open(os.path.join(ROOT, "robot_mpcs_amd", "csrc", "sources.txt")) as f:
        listed = f.read().split()
    assert "include/rmpc_assign_opt.h" in listed and "robot_mpcs_amd/csrc/rmpc_assign_opt.hpp" in listed


I_MAX, I_MIN = 2 ** 31 - 1, -2 ** 31
SIZES = (": need 1 <= B <= RMPC_ASSIGN_MAX_ROBOTS = 4096 and 1 <= T <= RMPC_ASSIGN_MAX_TARGETS = 1024")
G_BT = ": need 1 <= G and G*B*T <= INT_MAX"
BAD_SIZES = [(dict(B=0), SIZES), (dict(B=4097), SIZES), (dict(T=0), SIZES), (dict(T=1025), SIZES), (dict(B=I_MIN), SIZES),
             (dict(T=I_MAX), SIZES), (dict(G=0), G_BT), (dict(G=-1), G_BT), (dict(G=I_MIN), G_BT),
             (dict(G=512, B=4096, T=1024), G_BT), (dict(G=I_MAX, B=2, T=1), G_BT), (dict(G=0, B=0), SIZES)]


def test_work_bytes_is_host_only_and_refuses_bad_sizes(lib):
    """no device is touched (this test runs without one); the matrices take 4 G B T bytes behind the padded Qmax"""
    L = lib.load_library()
    wb = lib.assign_optimal_work_bytes
    assert wb(1, 1, 1) == 256 + 4 and wb(3, 5, 7) == 256 + 4 * 105 and wb(65, 2, 3) == 512 + 4 * 390
    assert wb(1, 4096, 1024) == 256 + 4 * 4096 * 1024 and wb(511, 4096, 1024) == 2048 + 4 * 511 * 4096 * 1024
    assert wb(I_MAX, 1, 1) == (4 * I_MAX + 255) // 256 * 256 + 4 * I_MAX
    assert wb(2, 3, 5) == wb(2, 5, 3)
    for bad, want in BAD_SIZES:
        a = dict(dict(G=1, B=4, T=4), **bad)
        assert L.rmpc_assign_optimal_work_bytes(a["G"], a["B"], a["T"]) == -1
        assert L.rmpc_last_error().decode() == "assign optimal work bytes" + want
        with pytest.raises(lib.RmpcError, match="assign optimal work bytes"):
            wb(a["G"], a["B"], a["T"])


P_ = 0x1000      # a host-side fake pointer: a refusal never dereferences it
ARGS = dict(G=1, B=4, T=6, cost=P_, scale=1024.0, assign=P_, total=None, count=None, steps=None, work=P_, bytes=1 << 20,
            stream=None)
NULL = "null argument"
SCALE = "assign optimal: scale must be finite and > 0"
REFUSALS = [(dict(cost=None), NULL), (dict(assign=None), NULL), (dict(work=None), NULL)]
REFUSALS += [(bad, "assign optimal" + want) for bad, want in BAD_SIZES]
REFUSALS += [(dict(scale=s), SCALE) for s in (0.0, -1.0, NAN, INF, -INF)]
REFUSALS += [(dict(bytes=256 + 4 * 24 - 1), "assign optimal: the workspace holds 351 bytes, 352 are needed "
              "(rmpc_assign_optimal_work_bytes)"),
             (dict(bytes=0), "assign optimal: the workspace holds 0 bytes, 352 are needed (rmpc_assign_optimal_work_bytes)"),
             (dict(bytes=-5), "assign optimal: the workspace holds -5 bytes, 352 are needed (rmpc_assign_optimal_work_bytes)"),
             # the first failing check speaks
             (dict(cost=None, B=0), NULL), (dict(B=0, scale=NAN), "assign optimal" + SIZES), (dict(scale=0.0, bytes=0), SCALE)]


@pytest.mark.parametrize("bad,want", REFUSALS, ids=[",".join("%s=%s" % kv for kv in b.items()) for b, _ in REFUSALS])
def test_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    L = lib.load_library()
    assert set(bad) <= set(ARGS)
    assert L.rmpc_assign_optimal_device(*dict(ARGS, **bad).values()) == -1
    assert L.rmpc_last_error().decode() == want


def test_wrapper_refuses_mismatched_tensors(lib):
    import torch
    cost = torch.zeros((2, 3, 4), dtype=torch.float64)
    ok = torch.zeros((2, 3), dtype=torch.int32)
    for c, a, kw in ((cost.float(), ok, {}), (cost[0, 0], ok[0], {}), (cost, ok[0], {}), (cost, ok.long(), {}),
                     (cost.transpose(1, 2), torch.zeros((2, 4), dtype=torch.int32), {}),
                     (cost, ok, dict(total=torch.zeros(2, dtype=torch.int32))),
                     (cost, ok, dict(count=torch.zeros(3, dtype=torch.int32))),
                     (cost, ok, dict(steps=torch.zeros(2, dtype=torch.int64)))):
        with pytest.raises(ValueError, match="assign_optimal_device"):
            lib.assign_optimal_device(c, a, **kw)
