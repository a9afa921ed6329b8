"""Any-angle routes (include/rmpc_any_angle.h), what needs no GPU: the integer cell walk of
tests/any_angle_reference.py against a plain statement of line of sight in exact rationals on every ordered pair of
cells of four small maps, hand-worked cases pinned as literals, the properties of the shortener on the store maps and
of the follower that looks ahead, the new header with its tables, and every refusal of the three entries."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from any_angle_cases import OCC, keep_flags, small_maps, store_case
from any_angle_reference import (OUTSIDE, TOO_LONG, chain_length, follow_visible_ref, occupancy, shorten_path, shorten_ref,
                                 touched, visible_pairs_ref, visible_plain, visible_walk)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = math.inf, math.nan
SYMBOLS = ["rmpc_grid_visible_device", "rmpc_grid_shorten_device", "rmpc_follow_visible_device"]
SEEDS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return _lib


# ---- the walk against the plain statement -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(small_maps()))
def test_walk_equals_the_plain_statement_on_every_ordered_pair(name):
    data = small_maps()[name]
    H, W = data.shape
    assert 7 <= H <= 9 and 7 <= W <= 9
    o = occupancy(data, OCC)
    seen = [0, 0]
    for a in range(H * W):
        for b in range(H * W):
            v = visible_walk(o, W, a, b)
            assert v == visible_plain(o, W, a, b), (name, divmod(a, W), divmod(b, W))
            seen[v] += 1
    assert seen[1] > H * W and (name == "empty") == (seen[0] == 0)


def test_walk_touches_exactly_the_squares_the_segment_meets():
    """on a 6 x 7 patch: the walk's cells are the closed squares the closed segment meets, the first apart, none twice"""
    from any_angle_reference import _meets
    H, W = 6, 7
    for a in range(H * W):
        for b in range(H * W):
            ends = (a // W, a % W, b // W, b % W)
            cells = list(touched(*ends))
            assert len(cells) == len(set(cells))
            assert set(cells) == {(r, c) for r in range(H) for c in range(W) if (r, c) != ends[:2] and _meets(*ends, r, c)}


# ---- cases worked by hand ---------------------------------------------------------------------------------------------
def grid_with(H, W, *occupied):
    g = np.zeros((H, W))
    for r, c in occupied:
        g[r, c] = 1.0
    return g


def sees(g, a, b):
    W = g.shape[1]
    v = visible_walk(occupancy(g), W, a[0] * W + a[1], b[0] * W + b[1])
    assert v == visible_plain(occupancy(g), W, a[0] * W + a[1], b[0] * W + b[1])
    return v


def test_an_axial_run_through_an_occupied_cell():
    assert list(touched(1, 0, 1, 4)) == [(1, 1), (1, 2), (1, 3), (1, 4)]
    assert list(touched(4, 2, 1, 2)) == [(3, 2), (2, 2), (1, 2)]
    assert sees(grid_with(3, 5), (1, 0), (1, 4)) and not sees(grid_with(3, 5, (1, 2)), (1, 0), (1, 4))
    assert sees(grid_with(3, 5, (0, 2), (2, 2)), (1, 0), (1, 4))          # the cells beside the run are not touched
    assert sees(grid_with(3, 5, (1, 2)), (1, 0), (1, 1)) and not sees(grid_with(3, 5, (1, 2)), (1, 4), (1, 1))


def test_the_pure_diagonal_counts_both_side_cells():
    """the dense planner takes the step between two occupied cells; line of sight does not, nor past one of them"""
    assert list(touched(0, 0, 1, 1)) == [(0, 1), (1, 0), (1, 1)]
    assert list(touched(2, 2, 0, 0)) == [(2, 1), (1, 2), (1, 1), (1, 0), (0, 1), (0, 0)]
    assert sees(grid_with(2, 2), (0, 0), (1, 1))
    assert not sees(grid_with(2, 2, (0, 1)), (0, 0), (1, 1)) and not sees(grid_with(2, 2, (1, 0)), (0, 0), (1, 1))
    assert not sees(grid_with(2, 2, (0, 1), (1, 0)), (0, 0), (1, 1))
    assert not sees(grid_with(2, 2, (0, 0), (1, 1)), (0, 1), (1, 0))


def test_one_row_and_three_columns_cross_a_corner():
    """from (2, 1) to (3, 4) the segment leaves (2, 2) through the corner (2.5, 2.5): (2, 3) and (3, 2) are touched too"""
    assert list(touched(2, 1, 3, 4)) == [(2, 2), (2, 3), (3, 2), (3, 3), (3, 4)]
    for cell, hidden in (((2, 2), True), ((2, 3), True), ((3, 2), True), ((3, 3), True), ((3, 4), True), ((3, 1), False),
                         ((2, 4), False), ((1, 2), False), ((4, 3), False)):
        assert sees(grid_with(6, 6, cell), (2, 1), (3, 4)) == (not hidden), cell
    # and mirrored: the same cells from the other end, the far end's own cell apart
    assert list(touched(3, 4, 2, 1)) == [(3, 3), (3, 2), (2, 3), (2, 2), (2, 1)]


def test_the_first_cell_is_exempt_and_the_last_is_not():
    g = grid_with(4, 4, (1, 1))
    assert sees(g, (1, 1), (1, 3)) and sees(g, (1, 1), (3, 2)) and sees(g, (1, 1), (1, 1))
    assert not sees(g, (1, 3), (1, 1)) and not sees(g, (3, 2), (1, 1)) and not sees(g, (0, 0), (1, 1))
    assert visible_pairs_ref(g, [5, 7, 5, -1, 3, 16], [7, 5, 5, 3, 16, 16]).tolist() == [1, 0, 1, -1, -1, -1]
    nan = grid_with(1, 3)
    nan[0, 1] = NAN                                                        # the planner's test: a NaN is occupied
    assert not sees(nan, (0, 0), (0, 2))


# ---- the shortener ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=SEEDS)
def store(request):
    from any_angle_cases import store_raw
    data, paths, lens = store_case(request.param)
    return data, paths, lens, shorten_ref(data, paths, lens), store_raw(request.param)


def test_shortened_store_routes_have_the_rules_properties(store):
    from robot_mpcs_amd.store import STORE as S
    data, paths, lens, (out, out_len, src), _ = store
    W = data.shape[1]
    o = occupancy(data)
    assert (lens > 1).all() and len(lens) == 64
    for b in range(64):
        L, n = lens[b], out_len[b]
        p, q, s = paths[b, :L].tolist(), out[b, :n].tolist(), src[b, :n].tolist()
        assert s[0] == 0 and s[-1] == L - 1 and all(y > x for x, y in zip(s, s[1:])) and q == [p[k] for k in s]
        assert all(y == x + 1 or visible_walk(o, W, p[x], p[y]) for x, y in zip(s, s[1:]))
        assert chain_length(q, W, S.cell) <= chain_length(p, W, S.cell) + 1e-12
        assert (out[b, n:] == -9).all() and (src[b, n:] == -9).all()
    share = out_len.sum() / lens.sum()
    print("kept share of the dense cells:", round(float(share), 3))
    assert share <= 0.5


def test_a_routes_own_steps_are_visible_on_the_raw_map_but_not_all_on_the_enlarged_one(store):
    """why examples/fleet_global_route.py lets its follower see on the raw map: a dense route rounds an
    enlarged corner by a diagonal whose side cell is occupied, which is no line of sight, and the follower's rule has no
    clause for the route's own next cell; on the map before the enlargement every step of such a route is visible"""
    data, paths, lens, _, raw = store
    W = data.shape[1]
    assert ((raw >= OCC) <= (data >= OCC)).all()
    hidden = {}
    for name, o in (("enlarged", occupancy(data)), ("raw", occupancy(raw))):
        hidden[name] = sum(not visible_walk(o, W, int(paths[b, k]), int(paths[b, k + 1])) for b in range(64) for k in range(lens[b] - 1))
    assert hidden["raw"] == 0 and hidden["enlarged"] > 0.05 * (lens - 1).sum(), hidden


def test_reach_one_is_the_identity_and_a_reach_bounds_every_skip(store):
    data, paths, lens, _, _ = store
    out, out_len, src = shorten_ref(data, paths, lens, reach=1)
    assert np.array_equal(out_len, lens)
    for b in range(64):
        assert np.array_equal(out[b, :lens[b]], paths[b, :lens[b]]) and src[b, :lens[b]].tolist() == list(range(lens[b]))
    _, n5, s5 = shorten_ref(data, paths, lens, reach=5)
    for b in range(64):
        assert np.diff(s5[b, :n5[b]]).max() <= 5
    assert n5.sum() >= store[3][1].sum()


def test_a_keep_flag_is_never_skipped(store):
    data, paths, lens, (_, free_len, _), _ = store
    keep = keep_flags(paths, lens)
    out, out_len, src = shorten_ref(data, paths, lens, keep=keep)
    assert keep.sum() > 64
    for b in range(64):
        s = src[b, :out_len[b]]
        assert set(np.flatnonzero(keep[b])) <= set(s.tolist())
        assert np.array_equal(out[b, :out_len[b]], paths[b, s])
    assert out_len.sum() > free_len.sum()


def test_short_paths_and_special_lengths():
    data = small_maps()["wall"]
    W = data.shape[1]
    paths = np.array([[3, 0, 0, 0], [3, 10, 0, 0], [0, 1, 2, 3], [0, 1, 99, 3], [0, -1, 2, 3], [5, 5, 5, 5], [7, 7, 7, 7],
                      [1, 1, 1, 2]], dtype=np.int32)
    lens = np.array([1, 2, 5, 4, 2, 0, -2, 4], dtype=np.int32)
    out, out_len, src = shorten_ref(data, paths, lens)
    assert out_len.tolist() == [1, 2, TOO_LONG, OUTSIDE, OUTSIDE, 0, -2, 2]
    assert out[0].tolist() == [3, -9, -9, -9] and out[1].tolist() == [3, 10, -9, -9] and src[1].tolist() == [0, 1, -9, -9]
    assert (out[2:7] == -9).all() and (src[2:7] == -9).all()
    assert out[7].tolist() == [1, 2, -9, -9] and src[7].tolist() == [0, 3, -9, -9]       # repeated cells collapse
    assert shorten_path(occupancy(data), W, [0, 1, 2, 3, 4])[1] == [0, 4]


# ---- the follower -----------------------------------------------------------------------------------------------------
X0, Y0, CELL = -9.0, -9.0, 0.45


def centre(c, W):
    return [X0 + (c % W) * CELL, Y0 + (c // W) * CELL, 0.0]


def follow(data, paths, lens, idx, pos, reach, look_ahead):
    B = len(lens)
    goal, blocked = np.full((B, 3), -7.0), np.full(B, -7, dtype=np.int32)
    follow_visible_ref(data, paths, lens, idx, pos, X0, Y0, CELL, reach, look_ahead, goal, blocked)
    return goal, blocked


def test_follower_on_an_empty_map_lands_on_the_end_of_its_reach():
    data = np.zeros((41, 41))
    paths = np.arange(41 * 3, 41 * 3 + 40, dtype=np.int32)[None, :].repeat(4, 0)
    lens = np.array([40, 40, 12, 0], dtype=np.int32)
    idx = np.array([0, 30, -5, 3], dtype=np.int32)
    pos = np.array([centre(41 * 3, 41)] * 4)
    for reach in (1, 16, 64):
        i = idx.copy()
        goal, blocked = follow(data, paths, lens, i, pos, reach, 1e3)
        want = [min(39, reach), min(39, 30 + reach), min(11, reach), 3]
        assert i.tolist() == want and blocked.tolist() == [0, 0, 0, -7]
        assert goal[:3].tolist() == [centre(paths[b, want[b]], 41) for b in range(3)] and (goal[3] == -7.0).all()


def test_follower_keeps_its_waypoint_when_it_sees_nothing_or_stands_outside():
    data = np.zeros((9, 9))
    data[:, 4] = 1.0                                                       # a wall between the robot and its route
    paths = np.array([[6, 15, 24, 33]] * 4, dtype=np.int32)
    lens = np.array([4] * 4, dtype=np.int32)
    idx = np.array([1, 1, 1, 9], dtype=np.int32)
    pos = np.array([centre(2, 9), [X0 - 5.0, Y0, 0.0], [NAN, Y0, 0.0], centre(6, 9)])
    goal, blocked = follow(data, paths, lens, idx, pos, 16, 1e3)
    assert idx.tolist() == [1, 1, 1, 3] and blocked.tolist() == [1, 1, 1, 0]
    assert goal.tolist() == [centre(15, 9)] * 3 + [centre(33, 9)]
    # the distance test alone: p[2] is two cells from the robot, p[3] three
    idx = np.zeros(4, dtype=np.int32)
    goal, blocked = follow(data, paths, lens, idx, np.array([centre(6, 9)] * 4), 16, 2.2 * CELL)
    assert idx.tolist() == [2] * 4 and blocked.tolist() == [0] * 4


def test_follower_index_is_monotone_and_the_goal_is_its_cells_centre():
    from any_angle_cases import scripted_positions
    data, paths, lens = store_case(0)
    W = data.shape[1]
    lens = lens.copy()
    lens[5] = 0
    pos = scripted_positions(paths, lens, W, X0, Y0, CELL, 30)
    idx = np.zeros(64, dtype=np.int32)
    goal = np.full((64, 3), -7.0)
    hidden = 0
    for t in range(30):
        before, blocked = idx.copy(), np.full(64, -7, dtype=np.int32)
        follow_visible_ref(data, paths, lens, idx, pos[t], X0, Y0, CELL, 16, 1.75, goal, blocked)
        assert (idx >= before).all() and (idx - before <= 16).all() and (idx < np.maximum(lens, 1)).all()
        for b in range(64):
            assert goal[b].tolist() == ([-7.0] * 3 if b == 5 else centre(paths[b, idx[b]], W))
        assert set(blocked.tolist()) <= {0, 1, -7} and blocked[5] == -7
        hidden += int((blocked == 1).sum())
    assert hidden > 0 and (idx > 0).sum() > 32


# ---- the header and the binding ---------------------------------------------------------------------------------------
def test_any_angle_symbols_are_declared_by_the_new_header_and_exported(lib):
    """the test that fails on the parent: the header, its tables and the three entries are new"""
    from robot_mpcs_amd import _abi
    assert lib.ANY_ANGLE_SYMBOLS == SYMBOLS == list(_abi.any_angle_prototypes)
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rmpc_any_angle.h")).read(), flags=re.S)
    code = re.sub(r"^[ \t]*#.*$", "", code, flags=re.M)
    assert sorted(set(re.findall(r"\b(rmpc_\w+)\s*\(", code))) == sorted(SYMBOLS)
    L = lib.load_library()
    for sym in SYMBOLS:
        fn = getattr(L, sym)
        assert (fn.restype, list(fn.argtypes)) == (_abi.any_angle_prototypes[sym][0], _abi.any_angle_prototypes[sym][1])
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    assert _abi.any_angle_prototypes[SYMBOLS[0]] == (i, [i, i, vp, d, i, vp, vp, vp, vp])
    assert _abi.any_angle_prototypes[SYMBOLS[1]] == (i, [i, i, vp, d, i, vp, vp, i, i] + [vp] * 6)
    assert _abi.any_angle_prototypes[SYMBOLS[2]] == (i, [i, vp, vp, i, vp, vp, i, i, i, vp, d, d, d, d, i, d, vp, vp, vp])
    assert _abi.any_angle_constants == {"RMPC_VISIBLE_MAX_REACH": 64} and lib.VISIBLE_MAX_REACH == 64
    assert lib.shorten_work_bytes(41, 41) == 4 * 41 * 2 and lib.shorten_work_bytes(2048, 2048) == 512 << 10
    assert lib.shorten_work_bytes(1, 32) == 4 and lib.shorten_work_bytes(3, 33) == 24
    # rmpc.h declares what it declared
    assert len(lib.EXPORTED_SYMBOLS) == 65 and _abi.constants["RMPC_VERSION"] == 201
    assert not set(SYMBOLS) & set(_abi.prototypes)
    with open(os.path.join(ROOT, "robot_mpcs_amd", "csrc", "sources.txt")) as f:
        listed = f.read().split()
    assert "include/rmpc_any_angle.h" in listed and "robot_mpcs_amd/csrc/rmpc_any_angle.hpp" in listed
    from robot_mpcs_amd import global_planner as gp
    assert issubclass(gp.VisibleFollower, gp.RouteFollower)
    assert all(callable(getattr(gp, n)) for n in ("visible", "shorten_routes", "route_lengths"))


P_ = 0x1000      # a host-side fake pointer: a refusal never dereferences it
I_MAX = 2 ** 31 - 1
NULL = "null argument"


def refusals(who, base, cases):
    ids = [",".join("%s=%s" % kv for kv in bad.items()) for bad, _ in cases]
    return pytest.mark.parametrize("bad,want", [(b, w if w == NULL else who + w) for b, w in cases], ids=ids), base


HW = ": need H, W >= 1"
B_LEN = ": need B, max_len >= 1 and B*max_len <= INT_MAX"


def large(H, W):
    return ": %dx%d map exceeds RMPC_GRID_LARGE_MAX_CELLS = 4194304 cells" % (H, W)


MAPS = [(dict(H=0), HW), (dict(W=0), HW), (dict(H=-3), HW), (dict(H=2049, W=2048), large(2049, 2048)),
        (dict(H=I_MAX, W=I_MAX), large(I_MAX, I_MAX))]

VISIBLE = dict(H=41, W=41, grid=P_, occ=0.8, P=5, a=P_, b=P_, out=P_, stream=None)
VISIBLE_REFUSALS = [(dict([(k, None)]), NULL) for k in ("grid", "a", "b", "out")] + MAPS
VISIBLE_REFUSALS += [(dict(P=0), ": need P >= 1"), (dict(P=-1), ": need P >= 1"), (dict(grid=None, P=0), NULL)]
mark, _ = refusals("grid visible", VISIBLE, VISIBLE_REFUSALS)


@mark
def test_visible_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    L = lib.load_library()
    assert set(bad) <= set(VISIBLE)
    assert L.rmpc_grid_visible_device(*dict(VISIBLE, **bad).values()) == -1
    assert L.rmpc_last_error().decode() == want


SHORTEN = dict(H=41, W=41, grid=P_, occ=0.8, B=4, path=P_, len=P_, max_len=64, reach=0, keep=None, out=P_ + 64, out_len=P_,
               src=None, work=P_, stream=None)
SHORTEN_REFUSALS = [(dict([(k, None)]), NULL) for k in ("grid", "path", "len", "out", "out_len", "work")] + MAPS
SHORTEN_REFUSALS += [(dict(B=0), B_LEN), (dict(max_len=0), B_LEN), (dict(B=-1), B_LEN), (dict(B=1 << 20, max_len=1 << 12), B_LEN),
                     (dict(reach=-1), ": reach must be >= 0 (0: the whole path)"),
                     (dict(out=P_), ": d_out may not be d_path"), (dict(H=0, B=0), HW)]
mark, _ = refusals("grid shorten", SHORTEN, SHORTEN_REFUSALS)


@mark
def test_shorten_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    L = lib.load_library()
    assert set(bad) <= set(SHORTEN)
    assert L.rmpc_grid_shorten_device(*dict(SHORTEN, **bad).values()) == -1
    assert L.rmpc_last_error().decode() == want


FOLLOW = dict(B=2, path=P_, len=P_, max_len=8, idx=P_, pos=P_, stride=3, H=41, W=41, grid=P_, occ=0.8, x0=0.0, y0=0.0, cell=0.45,
              reach=16, look_ahead=1.3, goal=P_, blocked=None, stream=None)
REACH = ": need 1 <= reach <= RMPC_VISIBLE_MAX_REACH = 64"
CELL_MSG, LOOK = ": cell must be finite and > 0", ": look_ahead must be finite and >= 2 cell"
STRIDE = ": need stride >= 2 and B*stride <= INT_MAX"
FOLLOW_REFUSALS = [(dict([(k, None)]), NULL) for k in ("path", "len", "idx", "pos", "grid", "goal")] + MAPS
FOLLOW_REFUSALS += [(dict(B=0), B_LEN), (dict(max_len=0), B_LEN), (dict(B=1 << 20, max_len=1 << 12), B_LEN),
                    (dict(stride=1), STRIDE), (dict(stride=-2), STRIDE), (dict(B=1 << 20, max_len=1, stride=1 << 12), STRIDE),
                    (dict(reach=0), REACH), (dict(reach=65), REACH), (dict(reach=-1), REACH)]
FOLLOW_REFUSALS += [(dict(cell=c), CELL_MSG) for c in (0.0, -0.45, NAN, INF)]
FOLLOW_REFUSALS += [(dict(look_ahead=v), LOOK) for v in (0.0, -1.0, NAN, INF, -INF, 0.89, math.nextafter(0.9, 0.0))]
mark, _ = refusals("follow visible", FOLLOW, FOLLOW_REFUSALS)


@mark
def test_follow_visible_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    L = lib.load_library()
    assert set(bad) <= set(FOLLOW)
    assert L.rmpc_follow_visible_device(*dict(FOLLOW, **bad).values()) == -1
    assert L.rmpc_last_error().decode() == want


def test_wrappers_refuse_mismatched_tensors(lib):
    import torch
    g = torch.zeros((4, 40), dtype=torch.float64)
    p, n = torch.zeros((2, 8), dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    work = torch.zeros(8, dtype=torch.int32)
    for kw in (dict(out=p[:, :4]), dict(keep=p[:1]), dict(src=p.T), dict(work=work[:7]), dict(work=torch.zeros((4, 4), dtype=torch.int32).T)):
        a = dict(dict(out=torch.zeros_like(p), keep=None, src=None, work=work), **kw)
        with pytest.raises(ValueError, match="grid_shorten_device"):
            lib.grid_shorten_device(g, p, n, a["out"], n.clone(), a["work"], keep=a["keep"], src=a["src"])
