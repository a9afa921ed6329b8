"""The rules of wide-window localisation (include/rmpc.h: rmpc_grid_min_pyramid_device, rmpc_scan_search_device;
DESIGN.md 21) as restated in tests/scan_search_reference.py: the pyramid against the literal window minimum, the wide
exhaustive rule against the matcher's, the property everything rests on (no candidate undercuts the key of a node above
it), a search on those bounds against the exhaustive rule on every launch the device is held to, what the wide window
recovers, and the entries' refusals.  tests/test_gpu_scan_search.py holds the device against the restatements."""
import ctypes as C
import math
import os
import types

import numpy as np
import pytest

import scan_search_cases as cases
from localization_cases import clear_poses, store_world
from localization_reference import edge_distance_ref, match_ref, wrap
from robot_mpcs_amd.store import STORE
from scan_search_reference import (Robot, match_wide_ref, min_pyramid_literal, min_pyramid_ref, node_bound_ref, node_m_min,
                                   scores_ref)


# ---- the pyramid ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.CPU_PYRAMIDS)
def test_pyramid_is_the_window_minimum(name):
    d2, sub, levels = cases.pyramid_case(name)
    pyr = min_pyramid_ref(d2, levels)
    assert pyr.dtype == np.int32 and np.array_equal(pyr[0], d2)
    assert np.array_equal(pyr, min_pyramid_literal(d2, levels))
    assert np.all(pyr[1:] <= pyr[:-1])
    if name == "12x9_sub3_beyond_the_map":                            # a window wider than the map: the map's minimum
        assert (1 << (levels - 1)) > max(d2.shape) and pyr[-1][0, 0] == d2.min()


# ---- the wide rule is the matcher's rule ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B, rays, lattice", [(8, 64, dict()), (2, 64, dict(nxy=15, step_xy=0.02, nth=15, step_th=0.005)),
                                              (5, 7, dict(nxy=2, step_xy=0.1, nth=0, step_th=0.0, min_hits=3))])
def test_wide_rule_equals_the_matchers_rule_within_15(B, rays, lattice):
    pose, t, _ = cases.store_robots(B, rays, 21, (0.2, 0.2, 0.05))
    t[0, ::2] = math.nan
    pose[B - 1, 1] += 40.0
    geom = cases.store_geom(**lattice)
    pts = cases.project(pose, t)
    want, got = match_ref(pose, pts, t, **geom), match_wide_ref(pose, pts, t, **geom)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    off = np.ones(B, np.int32)
    off[1] = 0
    got = match_wide_ref(pose, pts, t, active=off, **geom)
    assert got["best"][1] == -1 and got["score"][1] == got["score0"][1] == 0 and got["used"][1] == want["used"][1]
    assert np.array_equal(got["pose_out"][1], pose[1, :3])
    keep = np.arange(B) != 1
    for k in want:
        assert np.array_equal(got[k][keep], want[k][keep]), k


# ---- the property everything rests on --------------------------------------------------------------------------------------
def _border_robots(which):
    """(pose, points, ranges, geom, levels): a 13 x 13 x 3 lattice of steps wide enough that blocks straddle the border"""
    if which == "store":
        L = cases.launch("border")
        geom = dict(L["geom"], nxy=6, step_xy=0.11, nth=1, step_th=0.03, rot=cases.rotation_table(1, 0.03))
        return L["pose"], L["points"], L["ranges"], geom, 5
    L = cases.launch("12x9_map")
    pose = L["pose"].copy()
    pose[:, 0] = [-2.1, 3.6, 0.4, 1.0]                                # the little map spans x in [-2.25, 3.75], y in [-1.25, 3.25]
    pose[:, 1] = [0.3, 1.0, -1.2, 3.2]
    geom = dict(L["geom"], nxy=6, step_xy=0.13, nth=1, step_th=0.05, rot=cases.rotation_table(1, 0.05))
    return pose, cases.project(pose, L["ranges"]), L["ranges"], geom, 4


@pytest.mark.parametrize("which", ["store", "12x9"])
def test_no_leaf_undercuts_a_node_above_it(which):
    """For every node of every level of a 13 x 13 x 3 lattice with top_log2 2: its key (bound, m_min, 0) is at most the
    least key (score, m, k) of the leaves below it, and a leaf's bound is its score."""
    pose, points, ranges, geom, levels = _border_robots(which)
    pyr = min_pyramid_ref(geom["d2"], levels)
    nx, strict = 13, 0
    for b in range(len(pose)):
        r = Robot(pose[b], points[b], ranges[b], pyr, **geom)
        assert len(r.ux) >= geom["min_hits"]
        sc, m = scores_ref(pose[b], points[b], ranges[b], **geom)
        kk = np.arange(3 * nx * nx).reshape(3, nx, nx)
        for h in (2, 1, 0):
            side = 1 << h
            for jth in range(3):
                for b0 in range(0, nx, side):
                    for a0 in range(0, nx, side):
                        a1, b1 = min(a0 + side, nx) - 1, min(b0 + side, nx) - 1
                        v = int(node_bound_ref(r, [jth], [a0], [a1], [b0], [b1])[0])
                        mm = int(node_m_min(r, [jth], [a0], [a1], [b0], [b1])[0])
                        blk = (jth, slice(b0, b1 + 1), slice(a0, a1 + 1))
                        below = min(zip(sc[blk].ravel().tolist(), m[blk].ravel().tolist(), kk[blk].ravel().tolist()))
                        assert (v, mm, 0) <= below, (b, h, jth, a0, b0, v, mm, below)
                        assert mm == m[blk].min()
                        if h == 0:
                            assert v == below[0]
                        strict += int(h > 0 and v < sc[blk].min())
    assert strict > 0                                                 # (the bound is not the exact minimum everywhere)


# ---- a search on the bound is the exhaustive rule ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.LAUNCHES)
def test_search_equals_the_exhaustive_rule(name):
    want, got = cases.exhaustive(name), cases.searched(name)
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    matched = want["best"] >= 0
    L = cases.launch(name)
    K = (2 * L["geom"]["nxy"] + 1) ** 2 * (2 * L["geom"]["nth"] + 1)
    assert np.all(got["leaves"][matched] >= 1) and np.all(got["leaves"][matched] <= K) and np.all(got["leaves"][~matched] == 0)
    if matched.any():
        print("%s: leaves / K mean %.6f max %.6f" % (name, (got["leaves"][matched] / K).mean(), (got["leaves"][matched] / K).max()))


# ---- what the wide window recovers -------------------------------------------------------------------------------------------
# measured with this restatement: poses of 48 within two fine cells and 0.02 rad of the truth after the
# wide match and the fine match, and the failures at which the truth itself scores no better than the pose found
RECOVERY_MEASURED = dict(recovered=48, aliases=0)


def wide_recovery():
    rng = np.random.default_rng(0)
    raw, boxes, d2 = store_world()
    true = clear_poses(raw, 48, rng, STORE.clear_cells, 0.2)
    t = cases.store_scan(true, 64)
    prior = true + np.stack([rng.uniform(-1.5, 1.5, 48), rng.uniform(-1.5, 1.5, 48), rng.uniform(-0.4, 0.4, 48)], axis=1)
    wide = match_wide_ref(prior, cases.project(prior, t), t, **cases.store_geom(**cases.WIDE))
    assert np.all(wide["best"] >= 0)
    fine_geom = cases.store_geom(nxy=8, step_xy=0.0375, nth=6, step_th=0.0167)
    fine = match_wide_ref(wide["pose_out"], cases.project(wide["pose_out"], t), t, **fine_geom)
    at_truth = match_wide_ref(true, cases.project(true, t), t, **cases.store_geom(nxy=0, step_xy=0.0, nth=0, step_th=0.0))
    pos = np.hypot(*(fine["pose_out"][:, :2] - true[:, :2]).T)
    th = np.abs(wrap(fine["pose_out"][:, 2] - true[:, 2]))
    ok = (pos <= 2 * STORE.cell / 8) & (th <= 0.02)
    return ok, at_truth["score"] >= fine["score"], pos, th


def test_recovery_of_a_prior_far_outside_the_fine_lattice():
    """Store seed 0, the 48 poses of test_localization_cpu's recovery test; a prior within 1.5 m and 0.4 rad; the wide
    lattice 81 x 81 x 41 at 0.0375 m and 0.02 rad, then the fine 17 x 17 x 13 at 0.0375 m and 0.0167 rad at its result.
    Measured with the exhaustive restatement: RECOVERY_MEASURED.  The store's aisles repeat, so a prior may lock onto a
    neighbouring aisle; the gate is the measured count less two poses."""
    ok, alias, pos, th = wide_recovery()
    print("wide recovery: %d of 48 within %.4f m and 0.02 rad; of the %d others %d are aliases (the truth scores no better)"
          % (ok.sum(), 2 * STORE.cell / 8, (~ok).sum(), (alias & ~ok).sum()))
    print("errors of the others:", np.round(pos[~ok], 3).tolist(), np.round(th[~ok], 4).tolist())
    assert ok.sum() >= 40
    assert ok.sum() >= RECOVERY_MEASURED["recovered"] - 2


# ---- the entries: exported, and their refusals before any HIP call -------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return _lib


NAMES = {"rmpc_grid_min_pyramid_device", "rmpc_scan_search_work_bytes", "rmpc_scan_search_device"}


def test_new_entries_and_limits_are_exported(lib):
    assert NAMES <= set(lib.EXPORTED_SYMBOLS)
    L = C.CDLL(lib.LIB_PATH)
    assert all(hasattr(L, n) for n in NAMES)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rmpc.h")).read()
    assert all(("%s(" % n) in hdr for n in NAMES)
    assert "#define RMPC_SEARCH_MAX_N 127" in hdr and "} rmpc_scan_search;" in hdr
    assert (lib.SEARCH_MAX_N, lib.SEARCH_MAX_TOP, lib.SEARCH_MAX_LEVELS) == (127, 7, 12)
    # the search's struct begins with the matcher's
    n = len(lib.ScanMatchArgs._fields_)
    assert lib.ScanSearchArgs._fields_[:n] == lib.ScanMatchArgs._fields_
    assert all(getattr(lib.ScanSearchArgs, f).offset == getattr(lib.ScanMatchArgs, f).offset for f, _ in lib.ScanMatchArgs._fields_)
    src = open(os.path.join(os.path.dirname(lib.LIB_PATH), "sources.txt")).read()
    assert "robot_mpcs_amd/csrc/rmpc_search.hpp" in src


def test_refusals(lib):
    cases.check_refusals(lib, 0x1000)


def test_top_nodes_and_default_levels(lib):
    assert lib.scan_search_top_nodes(40, 20, 3) == 41 * 11 * 11 and lib.scan_search_top_nodes(127, 127, 0) == 255 ** 3
    assert lib.scan_search_top_nodes(0, 0, 7) == 1 and lib.scan_search_top_nodes(64, 1, 7) == 3 * 2 * 2
    assert cases.default_levels(3, 0.0375, 8, 0.45) == 4 and cases.default_levels(0, 0.0, 8, 0.45) == 2


def test_scan_searcher_refuses_bad_shapes_before_any_tensor(lib):
    from robot_mpcs_amd.utils.localization import ScanSearcher
    m = types.SimpleNamespace(sub=8, cell=0.45)
    kw = dict(nxy=40, step_xy=0.0375, nth=20, step_th=0.02)
    for bad, want in [(dict(nxy=128), "nxy"), (dict(nth=-1), "nth"), (dict(top_log2=8), "top_log2"), (dict(levels=0), "levels"),
                      (dict(levels=13), "levels")]:
        with pytest.raises(ValueError, match=want):
            ScanSearcher(m, **dict(kw, **bad))
