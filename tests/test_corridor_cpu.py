"""Safe corridors from the map (include/rmpc_corridor.h), what needs no GPU: the restatement on the
summed-area table against the one that slices the occupancy, on every free cell of four small maps and of the store;
the hand-worked cases pinned as literals; the rule's properties; the plane literals of one rectangle; the new header
with its tables; every refusal of the two entries."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from corridor_cases import FRAME, HAND, OCC, free_centres, hand_map, small_maps, special_map, store_frame, store_raw
from corridor_reference import (canonical_bits, corridor_plain, corridor_ref, count, dummy_plane, face_planes, grow, grow_plain,
                                occ_sums_ref, occupancy, seed_cell)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = math.inf, math.nan
SYMBOLS = ["rmpc_grid_occ_sums_device", "rmpc_grid_corridor_device"]
REACHES = (1, 2, 8)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return _lib


def all_maps():
    maps = {name: (g, FRAME) for name, g in small_maps().items()}
    maps.update({"store%d" % seed: (store_raw(seed), store_frame()) for seed in (0, 1, 2, 3)})
    return maps


MAPS = all_maps()


# ---- the two restatements ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MAPS))
@pytest.mark.parametrize("reach", REACHES)
def test_table_and_sliced_restatements_agree_on_every_free_cell(name, reach):
    grid, frame = MAPS[name]
    S, occ, pts = occ_sums_ref(grid, OCC), occupancy(grid, OCC), free_centres(grid, frame)
    a, b = np.full((len(pts), 1, 5, 4), -7.0), np.full((len(pts), 1, 5, 4), -7.0)
    ra, sa = corridor_ref(S, *frame, pts, reach, a, 1)
    rb, sb = corridor_plain(occ, *frame, pts, reach, b, 1)
    assert len(pts) == (~occ).sum() and (sa == 1).all() and np.array_equal(sa, sb)
    assert np.array_equal(ra, rb) and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert (a[:, :, 0] == -7.0).all() and (a[:, :, 1:] != -7.0).all()


def test_sums_are_the_counts_of_every_box_of_a_small_map():
    grid = special_map()
    S, occ = occ_sums_ref(grid, OCC), occupancy(grid, OCC)
    assert S.dtype == np.int32 and S.shape == (8, 10) and not S[0].any() and not S[:, 0].any()
    assert occ.sum() == 3 == S[-1, -1] and occ[1, 2] and occ[3, 4] and occ[4, 1] and not occ[5, 6] and not occ[2, 7]
    for ra in range(7):
        for rb in range(ra, 7):
            for ca in range(9):
                for cb in range(ca, 9):
                    assert count(S, ra, rb, ca, cb) == occ[ra:rb + 1, ca:cb + 1].sum()


# ---- the hand cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,reach,want", HAND)
def test_hand_cases(seed, reach, want):
    grid = hand_map()
    S = occ_sums_ref(grid, OCC)
    assert grow(S, *seed, reach)[0] == want == grow_plain(occupancy(grid, OCC), *seed, reach)[0]


def test_the_first_hand_case_takes_three_rounds():
    S = occ_sums_ref(hand_map(), OCC)
    assert grow(S, 2, 2, 8) == ((0, 4, 2, 3), 3) == grow_plain(occupancy(hand_map(), OCC), 2, 2, 8)


# ---- the properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MAPS))
@pytest.mark.parametrize("reach", REACHES)
def test_rectangles_have_the_rules_properties(name, reach):
    grid, _ = MAPS[name]
    S, occ = occ_sums_ref(grid, OCC), occupancy(grid, OCC)
    H, W = occ.shape
    for r, c in zip(*np.nonzero(~occ)):
        (r0, r1, c0, c1), rounds = grow(S, r, c, reach)
        assert 0 <= r0 <= r <= r1 < H and 0 <= c0 <= c <= c1 < W                       # the seed cell is inside
        assert not occ[r0:r1 + 1, c0:c1 + 1].any()                                    # every cell is free
        assert max(r - r0, r1 - r, c - c0, c1 - c) <= reach and rounds <= reach + 1   # no side beyond the reach
        # no direction can still advance: the next line is outside the map, beyond the reach or holds an occupied cell
        assert c1 + 1 >= W or c1 + 1 - c > reach or occ[r0:r1 + 1, c1 + 1].any()
        assert r1 + 1 >= H or r1 + 1 - r > reach or occ[r1 + 1, c0:c1 + 1].any()
        assert c0 - 1 < 0 or c - (c0 - 1) > reach or occ[r0:r1 + 1, c0 - 1].any()
        assert r0 - 1 < 0 or r - (r0 - 1) > reach or occ[r0 - 1, c0:c1 + 1].any()


def test_store_corridors_are_never_narrower_than_the_robot():
    """the issue's figures of the prototype: reach 8, from every free cell of the store's raw maps the shorter side is
    at least 3 cells (1.35 m against 2 r_body = 0.6 m) and no seed takes more than 9 rounds"""
    for seed in (0, 1, 2, 3):
        grid = store_raw(seed)
        S = occ_sums_ref(grid, OCC)
        for r, c in zip(*np.nonzero(grid < OCC)):
            (r0, r1, c0, c1), rounds = grow(S, r, c, 8)
            assert min(r1 - r0, c1 - c0) + 1 >= 3 and rounds <= 9


# ---- seeds and planes -------------------------------------------------------------------------------------------------
def test_seed_cells_round_half_to_even_and_refuse_what_is_not_a_cell():
    f = (0.0, 0.0, 0.5)
    assert seed_cell((0.25, 0.75, 0.0), 5, 7, *f) == (2, 0)           # 0.5 -> 0, 1.5 -> 2
    assert seed_cell((1.25, 1.25, 0.0), 5, 7, *f) == (2, 2)           # 2.5 -> 2
    assert seed_cell((-0.25, 0.0, 0.0), 5, 7, *f) == (0, 0)           # -0.5 -> -0.0, a cell
    assert seed_cell((3.25, 2.25, 0.0), 5, 7, *f) == (4, 6)           # 6.5 -> 6, 4.5 -> 4
    for p in ((3.3, 0.0), (0.0, 2.3), (-0.3, 0.0), (NAN, 0.0), (0.0, NAN), (INF, 0.0), (0.0, -INF), (1e300, 0.0)):
        assert seed_cell(p + (0.0,), 5, 7, *f) is None


def test_plane_literals_of_one_rectangle():
    got = face_planes((0, 4, 2, 3), -9.0, -9.0, 0.45)
    xlo, xhi, ylo, yhi = -9.0 + 1.5 * 0.45, -9.0 + 3.5 * 0.45, -9.0 + -0.5 * 0.45, -9.0 + 4.5 * 0.45
    want = np.array([[1.0, 0.0, 0.0, -xlo], [-1.0, 0.0, 0.0, xhi], [0.0, 1.0, 0.0, -ylo], [0.0, -1.0, 0.0, yhi]])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert not np.signbit(got[got == 0.0]).any()                                       # the zeros are +0.0
    assert got[:, 3].tolist() == [8.325, -7.425, 9.225, -6.975]
    # a point inside is on the positive side of every face, by its distance to the face
    p = np.array([-9.0 + 2 * 0.45, -9.0 + 2 * 0.45, 0.05, 1.0])
    assert np.allclose(got @ p, [0.225, 0.675, 1.125, 1.125], rtol=0, atol=1e-12)


def test_status_rect_and_dummy_planes_of_points_that_have_no_corridor():
    grid = hand_map()
    S = occ_sums_ref(grid, OCC)
    f = (0.0, 0.0, 0.5)
    pts = np.array([[[1.0, 1.0, 0.05], [2.0, 0.5, 0.05], [9.0, 1.0, 0.05], [NAN, 1.0, 0.05], [1.0, INF, 0.05]]])
    planes = np.full((1, 5, 4, 4), -7.0)
    rect, status = corridor_ref(S, *f, pts, 8, planes, 0)
    assert status.tolist() == [[1, 0, -1, -1, -1]]
    assert rect[0, 0].tolist() == [0, 4, 2, 3] and (rect[0, 1:] == -1).all()
    assert np.array_equal(planes[0, 0], face_planes((0, 4, 2, 3), *f))
    # HalfPlane(s + (20, 20, 0), s): the normal (-20, -20, 0), the plane through s + (20, 20, 0)
    assert planes[0, 1].tolist() == [[-20.0, -20.0, 0.0, 20.0 * 22.0 + 20.0 * 20.5]] * 4
    assert np.array_equal(planes[0, 2], np.tile(dummy_plane(pts[0, 2]), (4, 1))) and np.isfinite(planes[0, 2]).all()
    assert np.isnan(planes[0, 3, :, 0]).all() and np.isnan(planes[0, 3, :, 3]).all() and (planes[0, 3, :, 1] == -20.0).all()
    assert np.isnan(planes[0, 4, :, 1]).all() and np.isnan(planes[0, 4, :, 3]).all()
    assert (canonical_bits(planes[0, 4, :, 1]) == 0x7FF8000000000000).all()


# ---- the header and the binding ---------------------------------------------------------------------------------------
def test_corridor_symbols_are_declared_by_the_new_header_and_exported(lib):
    """the test that fails on the parent: the header, its tables and the two entries are new"""
    from robot_mpcs_amd import _abi
    assert lib.CORRIDOR_SYMBOLS == SYMBOLS == list(_abi.corridor_prototypes)
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rmpc_corridor.h")).read(), flags=re.S)
    code = re.sub(r"^[ \t]*#.*$", "", code, flags=re.M)
    assert sorted(set(re.findall(r"\b(rmpc_\w+)\s*\(", code))) == sorted(SYMBOLS)
    L = lib.load_library()
    for sym in SYMBOLS:
        fn = getattr(L, sym)
        assert (fn.restype, list(fn.argtypes)) == (_abi.corridor_prototypes[sym][0], _abi.corridor_prototypes[sym][1])
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    assert _abi.corridor_prototypes[SYMBOLS[0]] == (i, [i, i, vp, d, vp, vp])
    assert _abi.corridor_prototypes[SYMBOLS[1]] == (i, [i, i, vp, d, d, d, i, i, vp, i, i, i, vp, vp, vp, vp])
    assert _abi.corridor_constants == {"RMPC_CORRIDOR_MAX_REACH": 256} and lib.CORRIDOR_MAX_REACH == 256
    assert lib.corridor_sums_bytes(41, 41) == 4 * 42 * 42 and lib.corridor_sums_bytes(1, 1) == 16
    assert lib.corridor_sums_bytes(2048, 2048) == 4 * 2049 * 2049
    # rmpc.h declares what it declared
    assert len(lib.EXPORTED_SYMBOLS) == 65 and _abi.constants["RMPC_VERSION"] == 201
    assert not set(SYMBOLS) & set(_abi.prototypes)
    with open(os.path.join(ROOT, "robot_mpcs_amd", "csrc", "sources.txt")) as f:
        listed = f.read().split()
    assert "include/rmpc_corridor.h" in listed and "robot_mpcs_amd/csrc/rmpc_corridor.hpp" in listed
    from robot_mpcs_amd import utils
    from robot_mpcs_amd.utils.corridor import MapCorridors
    assert utils.MapCorridors is MapCorridors and callable(MapCorridors.step) and callable(MapCorridors.set_grid)


P_ = 0x1000      # a host-side fake pointer: a refusal never dereferences it
I_MAX = 2 ** 31 - 1
NULL = "null argument"


def refusals(who, cases):
    ids = [",".join("%s=%s" % kv for kv in bad.items()) for bad, _ in cases]
    return pytest.mark.parametrize("bad,want", [(b, w if w == NULL else who + w) for b, w in cases], ids=ids)


HW = ": need H, W >= 1"


def large(H, W):
    return ": %dx%d map exceeds RMPC_GRID_LARGE_MAX_CELLS = 4194304 cells" % (H, W)


MAP_REFUSALS = [(dict(H=0), HW), (dict(W=0), HW), (dict(H=-3), HW), (dict(H=2049, W=2048), large(2049, 2048)),
                (dict(H=I_MAX, W=I_MAX), large(I_MAX, I_MAX))]

SUMS = dict(H=41, W=41, grid=P_, occ=0.8, sums=P_, stream=None)
SUMS_REFUSALS = [(dict([(k, None)]), NULL) for k in ("grid", "sums")] + MAP_REFUSALS
SUMS_REFUSALS += [(dict(occ=v), ": occ_threshold must be finite") for v in (NAN, INF, -INF)] + [(dict(grid=None, H=0), NULL)]


@refusals("grid occ sums", SUMS_REFUSALS)
def test_sums_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    L = lib.load_library()
    assert set(bad) <= set(SUMS)
    assert L.rmpc_grid_occ_sums_device(*dict(SUMS, **bad).values()) == -1
    assert L.rmpc_last_error().decode() == want


CORRIDOR = dict(H=41, W=41, sums=P_, x0=-9.0, y0=-9.0, cell=0.45, B=4, N=20, points=P_, reach=8, nobst=7, slot0=2, planes=P_,
                rect=None, status=None, stream=None)
REACH = ": need 1 <= reach <= RMPC_CORRIDOR_MAX_REACH = 256"
SLOTS = ": need 0 <= slot0 and slot0 + 4 <= nobst"
BN, FITS = ": need B, N >= 1", ": B*N*nobst*4 must not exceed INT_MAX"
CELL_MSG, ORIGIN = ": cell must be finite and > 0", ": x0 and y0 must be finite"
CORRIDOR_REFUSALS = [(dict([(k, None)]), NULL) for k in ("sums", "points", "planes")] + MAP_REFUSALS
CORRIDOR_REFUSALS += [(dict(B=0), BN), (dict(N=0), BN), (dict(B=-1), BN), (dict(N=-20), BN)]
CORRIDOR_REFUSALS += [(dict(reach=v), REACH) for v in (0, -1, 257, I_MAX)]
CORRIDOR_REFUSALS += [(dict(slot0=-1), SLOTS), (dict(slot0=4), SLOTS), (dict(nobst=3, slot0=0), SLOTS), (dict(nobst=0, slot0=0), SLOTS),
                      (dict(slot0=I_MAX), SLOTS), (dict(nobst=-5, slot0=0), SLOTS)]
CORRIDOR_REFUSALS += [(dict(B=1 << 16, N=1 << 15), FITS), (dict(B=1 << 20, N=32, nobst=64), FITS), (dict(B=1 << 20, N=32, nobst=16, slot0=0), FITS)]
CORRIDOR_REFUSALS += [(dict(cell=v), CELL_MSG) for v in (0.0, -0.45, NAN, INF)]
CORRIDOR_REFUSALS += [(dict(x0=v), ORIGIN) for v in (NAN, INF)] + [(dict(y0=v), ORIGIN) for v in (NAN, -INF)]


@refusals("grid corridor", CORRIDOR_REFUSALS)
def test_corridor_entry_refuses_with_a_message_and_without_a_gpu(lib, bad, want):
    L = lib.load_library()
    assert set(bad) <= set(CORRIDOR)
    assert L.rmpc_grid_corridor_device(*dict(CORRIDOR, **bad).values()) == -1
    assert L.rmpc_last_error().decode() == want


def test_wrappers_and_class_refuse_mismatched_arguments(lib):
    import torch
    from robot_mpcs_amd.utils import MapCorridors
    g = torch.zeros((4, 6), dtype=torch.float64)
    for sums in (torch.zeros((4, 6), dtype=torch.int32), torch.zeros((5, 7), dtype=torch.int64), torch.zeros((7, 5), dtype=torch.int32).T):
        with pytest.raises(ValueError, match="grid_occ_sums_device"):
            lib.grid_occ_sums_device(g, sums)
    S, pts = torch.zeros((5, 7), dtype=torch.int32), torch.zeros((2, 3, 3), dtype=torch.float64)
    planes = torch.zeros((2, 3, 4, 4), dtype=torch.float64)
    for kw in (dict(planes=planes[:1]), dict(rect=torch.zeros((2, 3), dtype=torch.int32)), dict(status=torch.zeros((2, 4), dtype=torch.int32))):
        a = dict(dict(planes=planes, rect=None, status=None), **kw)
        with pytest.raises(ValueError, match="grid_corridor_device"):
            lib.grid_corridor_device(S, pts, a["planes"], 0.0, 0.0, 0.5, rect=a["rect"], status=a["status"])
    for kw in (dict(B=0), dict(reach=0), dict(reach=257), dict(heading=2), dict(slot0=1, nobst=4), dict(slot0=-1),
               dict(planes=torch.zeros((2, 3, 4, 4), dtype=torch.float32)), dict(planes=torch.zeros((2, 3, 3, 4), dtype=torch.float64))):
        a = dict(dict(B=2, N=3, grid=g, x0=0.0, y0=0.0, cell=0.5), **kw)
        with pytest.raises(ValueError, match="MapCorridors"):
            MapCorridors(**a)
