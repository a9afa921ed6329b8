"""Localisation on the device (rmpc_grid_edge_distance_device, rmpc_lidar_project_device, rmpc_scan_match_device,
ScanMatcher) against the numpy restatements of tests/localization_reference.py, bit for bit, each launch into poisoned
output buffers; and the closed loop of examples/fleet_store_localize.py with the matcher, with dead reckoning and
with the true pose."""
import math

import numpy as np
import pytest

from example_loader import load_example
from gpu_support import DEV, _t
from lidar_reference import scan_ref
from localization_cases import LIDAR, clear_poses, store_world
from localization_reference import edge_distance_ref, match_ref, project_ref
from robot_mpcs_amd.global_planner import shelf_map
from robot_mpcs_amd.store import STORE, store_map
from robot_mpcs_amd.utils.localization import rotation_table

pytestmark = pytest.mark.gpu

POISON = -559038737          # 0xDEADBEEF as an int32


@pytest.fixture(scope="module")
def rt():
    import torch
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return dict(torch=torch, lib=_lib)


# ---- edge distance -----------------------------------------------------------------------------------------------------
def _edge_cases():
    rng = np.random.default_rng(11)
    small = (rng.uniform(size=(7, 5)) < 0.35).astype(float)
    holed = small.copy()
    holed[3, 2] = math.nan
    holed[0, 0] = math.nan
    store = store_map(0)
    return {
        "7x5_sub3": (small, 0.5, 3, 40),
        "store_sub8": (store, 0.5, 8, 256),
        "128x128_sub2": (shelf_map(128, 128, seed=3, aisle=9, shelf=4, gap=6), 0.5, 2, 256),
        "store_sub1": (store, 0.5, 1, 30),
        "all_free": (np.zeros((9, 11)), 0.5, 4, 50),
        "all_occupied": (np.ones((9, 11)), 0.5, 4, 50),
        "nan_cells": (holed, 0.5, 3, 40),
        "widest_window": (small[:3, :4], 0.5, 8, 65535),      # ceil(sqrt(cap)) = 256 fine cells, wider than the map
        "threshold_and_cap_1": (rng.uniform(size=(6, 40)), 0.7, 7, 1),
    }


@pytest.mark.parametrize("name", list(_edge_cases()))
def test_edge_distance_is_the_restatement(rt, name):
    torch, lib = rt["torch"], rt["lib"]
    grid, occ, sub, cap = _edge_cases()[name]
    want = store_world()[2] if name == "store_sub8" else edge_distance_ref(grid, occ, sub, cap)
    H, W = grid.shape
    d2 = torch.full((H * sub, W * sub), POISON, dtype=torch.int32, device=DEV)
    lib.grid_edge_distance_device(_t(torch, grid), d2, occ, sub, cap)
    torch.cuda.synchronize()
    assert np.array_equal(d2.cpu().numpy(), want)


# ---- project -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweep", [(-math.pi, math.pi), (-math.pi + math.pi / 8, -math.pi / 8)])
def test_projection_is_the_restatement_and_the_scans_own_points(rt, sweep):
    torch, lib = rt["torch"], rt["lib"]
    rng = np.random.default_rng(4)
    raw, boxes, _ = store_world()
    B, R, stride = 37, 64, 8
    pose = np.zeros((B, stride))
    pose[:, :3] = clear_poses(raw, B, rng, 2, 0.2)
    pose[::7, 2] = 0.0
    kw = dict(angle_min=sweep[0], angle_max=sweep[1], max_range=10.0, offset=(0.4, 0.1), height=0.02)
    d_pose, d_boxes = _t(torch, pose), _t(torch, boxes)
    scan_pts = torch.full((B, R, 3), math.nan, dtype=torch.float64, device=DEV)
    scan_t = torch.full((B, R), math.nan, dtype=torch.float64, device=DEV)
    lib.lidar_scan_device(d_pose, scan_pts, d_boxes, None, ranges=scan_t, **kw)
    # the scan's pose and the scan's ranges: the scan's points, bit for bit
    pts = torch.full((B, R, 3), math.nan, dtype=torch.float64, device=DEV)
    lib.lidar_project_device(d_pose, scan_t, pts, **kw)
    torch.cuda.synchronize()
    assert torch.equal(pts, scan_pts) and bool((scan_t < 10.0).any())
    # a believed pose and any ranges: numpy's points to 1e-12 (sin and cos differ in the last bit)
    believed = pose.copy()
    believed[:, :3] += rng.uniform(-1, 1, (B, 3)) * [0.3, 0.3, 0.1]
    t = rng.uniform(0.0, 10.0, (B, R))
    pts.fill_(math.nan)
    lib.lidar_project_device(_t(torch, believed), _t(torch, t), pts, **kw)
    torch.cuda.synchronize()
    want = project_ref(believed, t, kw["angle_min"], kw["angle_max"], kw["offset"], kw["height"])
    assert np.abs(pts.cpu().numpy() - want).max() <= 1e-12


# ---- match -------------------------------------------------------------------------------------------------------------
def _store_geom(d2, sub=8, cap=256, nxy=3, step_xy=0.03, nth=4, step_th=0.01, min_hits=8):
    return dict(max_range=LIDAR["max_range"], d2=d2, H=STORE.H, W=STORE.W, sub=sub, cap=cap, x0=STORE.x0, y0=STORE.y0,
                cell=STORE.cell, nxy=nxy, step_xy=step_xy, nth=nth, step_th=step_th, rot=rotation_table(nth, step_th),
                min_hits=min_hits)


def _device_match(rt, pose, points, ranges, geom, optional=True):
    """one launch into poisoned buffers -> dict of numpy arrays (score0 and used only when given)"""
    torch, lib = rt["torch"], rt["lib"]
    B = len(pose)
    out = dict(pose_out=torch.full((B, 3), math.nan, dtype=torch.float64, device=DEV))
    for k in ("best", "score") + (("score0", "used") if optional else ()):
        out[k] = torch.full((B,), POISON, dtype=torch.int32, device=DEV)
    d_pose, d_pts, d_t = _t(torch, pose), _t(torch, points), _t(torch, ranges)
    d_d2, d_rot = _t(torch, geom["d2"], torch.int32), _t(torch, geom["rot"])
    a = lib.scan_match_args(d_pose, d_pts, d_t, d_d2, d_rot, out["pose_out"], out["best"], out["score"], geom["H"],
                            geom["W"], geom["sub"], geom["cap"], geom["x0"], geom["y0"], geom["cell"], geom["nxy"],
                            geom["step_xy"], geom["nth"], geom["step_th"], geom["max_range"], geom["min_hits"],
                            out.get("score0"), out.get("used"))
    lib.scan_match_device(a, B)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, want):
    for k, v in got.items():
        assert np.array_equal(v, want[k], equal_nan=True), (k, v, want[k])


def _store_case(B, rays, seed, prior=(0.08, 0.08, 0.03)):
    """true poses in the store, their scan, a prior beside each and the scan's ranges projected at the prior (numpy)"""
    rng = np.random.default_rng(seed)
    raw, boxes, _ = store_world()
    true = clear_poses(raw, B, rng, 2, 0.2)
    L = LIDAR
    _, t, _ = scan_ref(true, rays, L["angle_min"], L["angle_max"], L["max_range"], L["offset"], L["height"], boxes)
    pose = np.zeros((B, 8))
    pose[:, :3] = true + rng.uniform(-1, 1, (B, 3)) * prior
    pose[:, 3:] = rng.normal(size=(B, 5))
    return pose, t


def _project(pose, t):
    L = LIDAR
    with np.errstate(invalid="ignore"):
        return project_ref(pose, t, L["angle_min"], L["angle_max"], L["offset"], L["height"])


def test_match_of_one_candidate_and_of_fewer_candidates_than_threads(rt):
    d2 = store_world()[2]
    pose, t = _store_case(1, 1, 0)
    t[0, 0] = 2.5                                                     # (a single ray, made a hit whatever it met)
    geom = _store_geom(d2, nxy=0, step_xy=0.0, nth=0, step_th=0.0, min_hits=1)
    got = _device_match(rt, pose, _project(pose, t), t, geom)
    _same(got, match_ref(pose, _project(pose, t), t, **geom))
    assert got["best"][0] == 0 and got["used"][0] == 1 and got["score"][0] == got["score0"][0]
    assert np.array_equal(got["pose_out"][0], pose[0, :3] + 0.0)
    pose, t = _store_case(3, 5, 1)
    geom = _store_geom(d2, nxy=1, step_xy=0.05, nth=1, step_th=0.02, min_hits=2)
    got = _device_match(rt, pose, _project(pose, t), t, geom)
    _same(got, match_ref(pose, _project(pose, t), t, **geom))


def test_match_of_a_fleet_on_the_store_with_robots_that_cannot_match(rt):
    """B 64, R 64, the default lattice 7 x 7 x 9.  Robot 3: every ray a miss; 5: below min_hits; 9: a NaN pose (points
    projected at it are NaN); 12: NaN and infinite ranges among good ones; 20: the prior 40 m off, every end point
    outside the map, so the centre wins.  The others must not notice: their results equal those of a launch in which
    the odd robots are ordinary."""
    d2 = store_world()[2]
    pose, t = _store_case(64, 64, 2)
    geom = _store_geom(d2)
    plain = _device_match(rt, pose, _project(pose, t), t, geom)
    _same(plain, match_ref(pose, _project(pose, t), t, **geom))
    assert np.all(plain["best"] >= 0) and len(set(plain["best"].tolist())) > 8
    odd = [3, 5, 9, 12, 20]
    t[3] = LIDAR["max_range"]
    t[5, 5:] = LIDAR["max_range"]
    pose[9, 0] = math.nan
    t[12, ::3] = math.nan
    t[12, 1] = math.inf
    pose[20, 0] += 40.0
    pts = _project(pose, t)
    got = _device_match(rt, pose, pts, t, geom)
    _same(got, match_ref(pose, pts, t, **geom))
    assert got["best"][[3, 5, 9]].tolist() == [-1, -1, -1] and got["used"][[3, 5, 9]].tolist() == [0, 5, 0]
    assert got["best"][12] >= 0 and got["used"][12] < 64 - 22
    k0 = (4 * 7 + 3) * 7 + 3
    assert got["best"][20] == k0 and got["score"][20] == got["used"][20] * 256 == got["score0"][20]
    keep = np.setdiff1d(np.arange(64), odd)
    for k in got:
        assert np.array_equal(got[k][keep], plain[k][keep]), k
    # score0 and used are optional: the other outputs do not change
    bare = _device_match(rt, pose, pts, t, geom, optional=False)
    assert set(bare) == {"pose_out", "best", "score"}
    _same(bare, got)


def test_match_of_the_largest_lattice(rt):
    """B 5, R 64, nxy = nth = 15: 29 791 candidates, 117 per thread"""
    d2 = store_world()[2]
    pose, t = _store_case(5, 64, 3, prior=(0.25, 0.25, 0.06))
    geom = _store_geom(d2, nxy=15, step_xy=0.02, nth=15, step_th=0.005)
    pts = _project(pose, t)
    got = _device_match(rt, pose, pts, t, geom)
    _same(got, match_ref(pose, pts, t, **geom))
    assert np.all(got["best"] >= 0) and np.all(got["score"] <= got["score0"])


def test_match_with_more_rays_than_threads_and_on_an_empty_map(rt):
    d2 = store_world()[2]
    pose, t = _store_case(4, 300, 4)
    geom = _store_geom(d2, nxy=2, step_xy=0.04, nth=2, step_th=0.01)
    pts = _project(pose, t)
    got = _device_match(rt, pose, pts, t, geom)
    _same(got, match_ref(pose, pts, t, **geom))
    assert np.all(got["used"] > 256)
    # an empty map: every score is used x cap, the tie goes to the centre and the prior comes back
    geom["d2"] = np.full_like(d2, 256)
    got = _device_match(rt, pose, pts, t, geom)
    _same(got, match_ref(pose, pts, t, **geom))
    assert np.all(got["best"] == (2 * 5 + 2) * 5 + 2) and np.array_equal(got["score"], got["used"] * 256)
    assert np.array_equal(got["pose_out"], pose[:, :3] + 0.0)
    # a coarser table of another map and sub, with end points beyond its edge
    small = np.zeros((9, 12))
    small[4:6, 3:9] = 1.0
    geom = dict(_store_geom(edge_distance_ref(small, 0.5, 3, 20), sub=3, cap=20, nxy=3, step_xy=0.2, nth=1, step_th=0.05),
                H=9, W=12, x0=-2.0, y0=-1.0, cell=0.5)
    got = _device_match(rt, pose, pts, t, geom)
    _same(got, match_ref(pose, pts, t, **geom))


# ---- ScanMatcher -------------------------------------------------------------------------------------------------------
def test_scan_matcher_step_on_a_side_stream_equals_the_default_stream(rt):
    torch, lib = rt["torch"], rt["lib"]
    from robot_mpcs_amd.utils.localization import ScanMatcher
    raw, boxes, d2 = store_world()
    B = 64
    pose, t = _store_case(B, 64, 6)
    L = LIDAR
    make = lambda: ScanMatcher(B, STORE.H, STORE.W, STORE.x0, STORE.y0, STORE.cell, L["rays"], L["max_range"], L["offset"],
                               L["height"], L["angle_min"], L["angle_max"], device=DEV)
    d_pose, d_t, d_raw = _t(torch, pose), _t(torch, t), _t(torch, raw)
    names = ("pose_out", "best", "score", "score0", "used", "points")

    def poisoned(m):
        m.d2.fill_(POISON)
        m.pose_out.fill_(math.nan)
        m.points.fill_(math.nan)
        for k in ("best", "score", "score0", "used"):
            getattr(m, k).fill_(POISON)
        return m

    a = poisoned(make())
    a.set_map(d_raw, 0.5)
    assert a.step(d_pose, d_t) is a.pose_out
    torch.cuda.synchronize()
    ref = {k: getattr(a, k).cpu().numpy() for k in names}
    assert np.array_equal(a.d2.cpu().numpy(), d2)
    # the match of the points the device projected: the restatement, bit for bit
    want = match_ref(pose, ref["points"], t, **_store_geom(d2))
    for k in want:
        assert np.array_equal(ref[k], want[k]), k
    assert np.all(ref["best"] >= 0)
    b = poisoned(make())
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    b.set_map(d_raw, 0.5, stream=side.cuda_stream)
    b.step(d_pose, d_t, stream=side.cuda_stream)
    side.synchronize()
    for k in names + ("d2",):
        assert np.array_equal(getattr(b, k).cpu().numpy(), getattr(a, k).cpu().numpy()), k


# ---- closed loop -------------------------------------------------------------------------------------------------------
def test_closed_loop_needs_and_has_the_matcher(rt):
    """64 boxers cross the store on routes followed at the ESTIMATED pose (examples/fleet_store_localize.py, seed 0).
    The true-pose run (the loop of fleet_store_lidar.py) gives the last arrival A; the matcher and dead reckoning then
    run ceil(1.35 A) steps.  Gates with the matcher: the lidar loop's safety gates (at most 1 % of the robot-steps
    failed, no base centre inside a shelf, the end link never within 0.5 r_body of a shelf); the estimate within half
    a cell (0.225 m) of the truth on every robot-step; at least 0.95 of the true-pose run's arrivals, the last within
    1.35 A.  With dead reckoning the final mean error exceeds ten times the matcher's: the loop needs the matcher.
    MI355X measurements: DESIGN.md 17."""
    ex = load_example("fleet_store_localize")
    truth = ex.run(B=64, steps=200, seed=0, mode="true-pose")
    print(truth)
    assert truth["routes"] == 64 and truth["arrival_share"] >= 0.9, truth
    steps = math.ceil(1.35 * truth["arrival_step_max"])
    r = ex.run(B=64, steps=steps, seed=0, mode="match")
    print(r)
    assert r["fused"] and r["routes"] == 64, r
    assert r["failed_share"] <= 0.01, r
    assert r["base_inside"] == 0 and r["min_base_clearance_m"] > 0.0, r
    assert r["min_ee_clearance_m"] >= 0.5 * r["r_body"], r
    assert r["pos_err_max_m"] <= 0.5 * STORE.cell, r
    assert r["arrivals"] >= 0.95 * truth["arrivals"], (r, truth)
    assert r["arrival_step_max"] <= 1.35 * truth["arrival_step_max"], (r, truth)
    dead = ex.run(B=64, steps=steps, seed=0, mode="dead-reckoning")
    print(dead)
    assert dead["pos_err_final_mean_m"] > 10.0 * r["pos_err_final_mean_m"], (dead, r)
