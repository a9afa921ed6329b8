"""The lidar on the device (rmpc_lidar_scan_device, rmpc_plan_points_device) and LidarPlanes (scan -> seeds -> FSD)
against the numpy restatement of tests/lidar_reference.py and oracle/fsd_numpy.py; the refusals of the C ABI; stream
and device selection; the closed loop of examples/fleet_store_lidar.py with and without the lidar."""
import ctypes as C
import math

import numpy as np
import pytest

from example_loader import load_example
from gpu_support import DEV, _t
from lidar_reference import plan_points_ref, scan_ref

pytestmark = pytest.mark.gpu

SWEEPS = {"full": (-math.pi, math.pi), "sector": (-math.pi + math.pi / 8, -math.pi / 8)}
# a last-bit difference of d (the device's and numpy's sin / cos) moves the circle hit t = -b - sqrt(b^2 - c) by about
# |b| eps / sqrt(b^2 - c): unbounded at tangency.  Rays on which that exceeds 1e-13 m are excluded as well as the rays
# within 1e-9 of a corner or a tangent.
EPS = 2.3e-16


@pytest.fixture(scope="module")
def rt():
    import torch
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return dict(torch=torch, lib=_lib)


def _world(rng, nbox, ncircle):
    boxes = np.concatenate([rng.uniform(-10, 10, (nbox, 2)), rng.uniform(0.1, 2.0, (nbox, 2))], 1)
    circles = np.concatenate([rng.uniform(-10, 10, (ncircle, 2)), rng.uniform(0.1, 1.0, (ncircle, 1))], 1)
    return boxes, circles


def _poses(rng, B, stride=8, zero_heading=True):
    pose = rng.normal(size=(B, stride))
    pose[:, :2] = rng.uniform(-10, 10, (B, 2))
    pose[:, 2] = rng.uniform(-math.pi, math.pi, B)
    if zero_heading:
        pose[::7, 2] = 0.0    # heading 0: the full sweep then holds a ray with sin = 0 exactly
    return pose


def _fsd_ambiguous(points, seed, K, max_radius, tol=1e-9):
    """A stage whose greedy choices a last-bit difference of the cloud may change: a point within tol of max_radius,
    two nearest candidates within tol, or a remaining point within tol of a plane (the on-or-behind test v <= 0).  A
    ray that meets a flat face at the seed's perpendicular foot puts the whole face on the first plane."""
    from oracle.fsd_numpy import dot3, half_plane
    d = np.linalg.norm(points - seed, axis=1)
    if np.any(np.abs(d - max_radius) <= tol):
        return True
    order = np.argsort(d, kind="stable")
    pts, dd = points[order][d[order] < max_radius], d[order][d[order] < max_radius]
    n = 0
    while len(pts) and n < K:
        if len(dd) > 1 and dd[1] - dd[0] <= tol:
            return True
        c = half_plane(pts[0], seed)
        v = np.array([dot3(c[:3], q) + c[3] for q in pts])
        if np.any(np.abs(v[1:]) <= tol * np.linalg.norm(c[:3])):
            return True
        keep = ~(v <= 0)
        pts, dd, n = pts[keep], dd[keep], n + 1
    return False


def _sensitive(pose, R, amin, amax, rng_, offset, circles, t_ref):
    """rays whose circle hit a last-bit change of the direction moves by more than 1e-13 m"""
    ox = pose[:, 0] + offset[0] * np.cos(pose[:, 2]) - offset[1] * np.sin(pose[:, 2])
    oy = pose[:, 1] + offset[0] * np.sin(pose[:, 2]) + offset[1] * np.cos(pose[:, 2])
    ang = (pose[:, 2:3] + amin) + np.arange(R)[None, :] * ((amax - amin) / R)
    dx, dy = np.cos(ang), np.sin(ang)
    bad = np.zeros(t_ref.shape, dtype=bool)
    for cx, cy, r in circles:
        ux, uy = ox[:, None] - cx, oy[:, None] - cy
        bb = dx * ux + dy * uy
        disc = bb * bb - ((ux * ux + uy * uy) - r * r)
        hit = np.abs(t_ref - (-bb - np.sqrt(np.maximum(disc, 0.0)))) <= 1e-9
        bad |= hit & (disc >= 0) & (np.hypot(ux, uy) * EPS * np.abs(bb) > 1e-13 * np.sqrt(np.maximum(disc, 1e-300)))
    return bad


def _scan(rt, pose, R, amin, amax, max_range, offset, boxes, circles, stream=None):
    torch = rt["torch"]
    B = pose.shape[0]
    pts = torch.full((B, R, 3), float("nan"), dtype=torch.float64, device=DEV)
    rng_ = torch.full((B, R), float("nan"), dtype=torch.float64, device=DEV)
    rt["lib"].lidar_scan_device(_t(torch, pose), pts, _t(torch, boxes), _t(torch, circles), amin, amax, max_range,
                                offset, 0.02, ranges=rng_, stream=stream)
    torch.cuda.synchronize()
    return pts.cpu().numpy(), rng_.cpu().numpy()


@pytest.mark.parametrize("B,R,sweep", [(37, 1, "full"), (37, 64, "full"), (37, 257, "full"), (4099, 1, "full"),
                                       (4099, 64, "full"), (4099, 257, "full"), (37, 64, "sector"),
                                       (4099, 64, "sector")])
def test_scan_matches_restatement(rt, B, R, sweep):
    rng = np.random.default_rng(B * 1000 + R)
    boxes, circles = _world(rng, 300, 20)
    pose = _poses(rng, B)
    amin, amax = SWEEPS[sweep]
    offset, max_range = (0.4, 0.15), 9.0
    pts, rng_ = _scan(rt, pose, R, amin, amax, max_range, offset, boxes, circles)
    ref_p, ref_t, near = scan_ref(pose, R, amin, amax, max_range, offset, 0.02, boxes, circles)
    excl = near | _sensitive(pose, R, amin, amax, max_range, offset, circles, ref_t)
    assert excl.mean() < 0.005, excl.mean()
    keep = ~excl
    assert np.all(np.isfinite(pts)) and np.all(pts[:, :, 2] == 0.02)
    assert np.abs(rng_ - ref_t)[keep].max() <= 1e-12
    assert np.abs(pts - ref_p).max(axis=2)[keep].max() <= 1e-12
    # the scan sees the world: some rays hit, some miss, and every hit is closer than the range
    assert 0 < (ref_t < max_range).sum() < ref_t.size and np.all(rng_ <= max_range)


def test_plan_points_match_restatement(rt):
    torch = rt["torch"]
    rng = np.random.default_rng(5)
    for B, N, nvar in ((37, 10, 10), (4099, 10, 10), (5, 1, 3)):
        pose = _poses(rng, B)
        z = rng.normal(size=(B, N, nvar)) * 4.0
        ef = rng.choice(np.array([-7, -1, 0, 1, 2], np.int32), B)
        for zz, ee in ((None, None), (z, None), (z, ef), (None, ef)):
            out = torch.full((B, N, 3), float("nan"), dtype=torch.float64, device=DEV)
            rt["lib"].plan_points_device(_t(torch, pose), out, None if zz is None else _t(torch, zz),
                                         None if ee is None else _t(torch, ee, torch.int32), (0.4, -0.1), 0.02)
            torch.cuda.synchronize()
            ref = plan_points_ref(pose, N, zz, ee, (0.4, -0.1), 0.02)
            assert np.abs(out.cpu().numpy() - ref).max() <= 1e-13


def _store(seed, big):
    from robot_mpcs_amd.global_planner import shelf_map
    from robot_mpcs_amd.utils.lidar import boxes_from_grid
    H = 128 if big else 41
    cell = 0.15 if big else 0.45
    raw = shelf_map(H, H, seed=seed, aisle=9 if big else 6, shelf=4 if big else 2, gap=6 if big else 5)
    x0 = -0.5 * (H - 1) * cell
    return raw, boxes_from_grid(raw, x0, x0, cell), x0, cell


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("big", [False, True])
def test_lidar_planes_step_matches_restated_chain(rt, K, big):
    from oracle.fsd_numpy import free_space_decomposition
    from robot_mpcs_amd.utils.lidar import LidarPlanes
    torch = rt["torch"]
    rng = np.random.default_rng(K + 10 * big)
    raw, boxes, x0, cell = _store(K, big)
    H = raw.shape[0]
    free = np.flatnonzero(raw.ravel() < 0.5)
    B, N, nvar = 96, 10, 10
    c = rng.choice(free, B)
    pose = _poses(rng, B, zero_heading=False)
    pose[:, 0], pose[:, 1] = x0 + (c % H) * cell, x0 + (c // H) * cell
    z = rng.normal(scale=0.05, size=(B, N, nvar))
    z[:, :, :3] += pose[:, None, :3]
    ef = rng.choice(np.array([-7, 0, 1], np.int32), B)
    lp = LidarPlanes(B, N, K, boxes=boxes, device=DEV)
    for zz, ee in ((None, None), (z, ef)):
        planes = lp.step(_t(torch, pose), None if zz is None else _t(torch, zz),
                         None if ee is None else _t(torch, ee, torch.int32)).cpu().numpy()
        pts, t, near = scan_ref(pose, 64, -math.pi, math.pi, 10.0, (0.4, 0.0), 0.02, boxes)
        seeds = plan_points_ref(pose, N, zz, ee, (0.4, 0.0), 0.02)
        assert np.abs(lp.seeds.cpu().numpy() - seeds).max() <= 1e-13
        keep = ~near.any(axis=1)          # a robot with a ray near a corner: its cloud may differ in one point
        assert keep.mean() > 0.9, keep.mean()
        assert np.abs(lp.points.cpu().numpy() - pts)[keep].max() <= 1e-12
        ref = np.stack([[free_space_decomposition(pts[b], seeds[b, k], K, 5.0) for k in range(N)] for b in range(B)])
        amb = np.array([[_fsd_ambiguous(pts[b], seeds[b, k], K, 5.0) for k in range(N)] for b in range(B)])
        assert amb.mean() < 0.02, amb.mean()
        same = keep[:, None] & ~amb
        assert np.allclose(planes[same], ref[same], rtol=1e-12, atol=1e-11)
        # real planes: the nearest shelf face is within the FSD radius of every robot in the store
        assert np.all(np.abs(planes[keep][:, :, 0, :2]).max(axis=2) < 5.0)


def test_refusals(rt):
    torch = rt["torch"]
    lib = rt["lib"]
    L = lib.load_library()
    B, R, N = 4, 8, 3
    pose = torch.zeros((B, 8), dtype=torch.float64, device=DEV)
    pts = torch.zeros((B, R, 3), dtype=torch.float64, device=DEV)
    boxes = torch.tensor([[1.0, 0.0, 0.5, 0.5]], dtype=torch.float64, device=DEV)
    circles = torch.tensor([[0.0, 2.0, 0.5]], dtype=torch.float64, device=DEV)

    def scan(B_=B, **kw):
        a = lib.lidar_args(pose, pts, boxes, circles)
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.rmpc_lidar_scan_device(B_, C.byref(a), None)
        return rc, L.rmpc_last_error().decode()

    assert scan()[0] == 0
    size = C.sizeof(lib.LidarArgs)
    bad = [dict(struct_size=size + 8), dict(struct_size=size - 8), dict(rays=0), dict(B_=0), dict(pose_stride=2),
           dict(range=0.0), dict(range=-1.0), dict(range=math.inf), dict(range=math.nan), dict(pose=None),
           dict(points=None), dict(boxes=None), dict(circles=None), dict(nbox=-1), dict(ncircle=-1),
           dict(B_=1 << 20, rays=1 << 12), dict(nbox=1 << 30), dict(ncircle=1 << 30)]
    for kw in bad:
        rc, msg = scan(**kw)
        assert rc == -1 and msg, kw
    assert L.rmpc_lidar_scan_device(B, None, None) == -1
    # a NULL shape pointer is fine when its count is 0
    assert scan(boxes=None, nbox=0, circles=None, ncircle=0)[0] == 0

    seeds = torch.zeros((B, N, 3), dtype=torch.float64, device=DEV)
    z = torch.zeros((B, N, 10), dtype=torch.float64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())

    def plan(B_=B, N_=N, z_=z, nvar=10, pose_=pose, stride=8, out=seeds):
        rc = L.rmpc_plan_points_device(B_, N_, None if z_ is None else p(z_), nvar, None,
                                       None if pose_ is None else p(pose_), stride, 0.4, 0.0, 0.02,
                                       None if out is None else p(out), None)
        return rc, L.rmpc_last_error().decode()

    assert plan()[0] == 0 and plan(z_=None)[0] == 0
    for kw in (dict(pose_=None), dict(out=None), dict(B_=0), dict(N_=0), dict(stride=2), dict(nvar=2),
               dict(B_=1 << 16, N_=1 << 16), dict(B_=1 << 12, N_=1 << 10, nvar=1 << 10), dict(B_=1 << 29, stride=8)):
        rc, msg = plan(**kw)
        assert rc == -1 and msg, kw
    torch.cuda.synchronize()


def _chain(rt, lp, pose, z, ef, stream):
    torch = rt["torch"]
    with torch.cuda.stream(stream):
        lp.step(pose, z, ef)
    stream.synchronize()
    return lp.points.cpu().numpy(), lp.seeds.cpu().numpy(), lp.planes.cpu().numpy()


def _chain_inputs(rt):
    torch = rt["torch"]
    rng = np.random.default_rng(3)
    raw, boxes, x0, cell = _store(2, False)
    B, N, K = 300, 10, 4
    free = np.flatnonzero(raw.ravel() < 0.5)
    c = rng.choice(free, B)
    pose = _poses(rng, B)
    pose[:, 0], pose[:, 1] = x0 + (c % 41) * cell, x0 + (c // 41) * cell
    z = rng.normal(scale=0.1, size=(B, N, 10))
    z[:, :, :3] += pose[:, None, :3]
    ef = rng.choice(np.array([-1, 0, 1], np.int32), B)
    return (B, N, K, boxes), (_t(torch, pose), _t(torch, z), _t(torch, ef, torch.int32))


def test_stream_ordering(rt):
    from robot_mpcs_amd.utils.lidar import LidarPlanes
    torch = rt["torch"]
    (B, N, K, boxes), args = _chain_inputs(rt)
    lp = LidarPlanes(B, N, K, boxes=boxes, device=DEV)
    ref = _chain(rt, lp, *args, torch.cuda.default_stream(0))
    side = torch.cuda.Stream(device=0)
    for _ in range(3):
        lp.planes.fill_(float("nan"))
        lp.points.fill_(float("nan"))
        got = _chain(rt, lp, *args, side)
        assert all(np.array_equal(a, b) for a, b in zip(ref, got))


def test_device_selection_on_a_second_gpu(rt):
    """scan, seeds and FSD (rmpc_free_space_device now selects the device of d_points) on cuda:1 while cuda:0 is
    current"""
    from robot_mpcs_amd.utils.lidar import LidarPlanes
    torch = rt["torch"]
    if torch.cuda.device_count() < 2:
        pytest.skip("device selection: one GPU visible")
    (B, N, K, boxes), args = _chain_inputs(rt)
    ref = _chain(rt, LidarPlanes(B, N, K, boxes=boxes, device=DEV), *args, torch.cuda.default_stream(0))
    torch.cuda.set_device(0)
    lp1 = LidarPlanes(B, N, K, boxes=boxes, device="cuda:1")
    args1 = tuple(a.to("cuda:1") for a in args)
    with torch.cuda.device(0):
        lp1.step(*args1)
    torch.cuda.synchronize(1)
    got = (lp1.points.cpu().numpy(), lp1.seeds.cpu().numpy(), lp1.planes.cpu().numpy())
    assert all(np.array_equal(a, b) for a, b in zip(ref, got))


def test_closed_loop_planes_keep_boxers_off_the_shelves(rt):
    """256 boxers (boxerMpc.yaml, K = 4 planes per stage, r_body = 0.6) cross a 41 x 41 store of 0.45 m cells on routes
    from the map enlarged by one cell, with the lidar planes as hard constraints of the end link
    (examples/fleet_store_lidar.py, defaults, seed 0).  First MI355X measurement over 1200 control steps: all 256
    routes found, all 256 end links within ARRIVE_TOL["cfg3"] (0.35 m) of their final goal by control step 101 (p50 68,
    p90 84), 2 failed solves in 307 200 robot-steps, least end-link-to-shelf distance 0.581 m (p10 0.603 m), least
    base-centre distance 0.185 m.  Without the lidar (same seed): arrivals alike (max 101), least end-link distance
    0.029 m, 23 robots' end links within 0.5 r_body, 3 base centres inside a shelf box.
    Gate: every route found, SHARE = 0.9 of the robots arrived by STEPS = 137 (1.35 x the last arrival), at most 1 % of
    the robot-steps failed, no base centre inside a shelf box, the end link never within 0.5 r_body of a shelf; and the
    same seed without the lidar brings some end link within 0.5 r_body of a shelf (the planes, not the route, keep the
    robots off)."""
    SHARE, STEPS = 0.9, 137
    ex = load_example("fleet_store_lidar")
    r = ex.run(B=256, steps=STEPS, seed=0)
    print(r)
    assert r["fused"]
    assert r["routes"] == 256, r
    assert r["arrival_share"] >= SHARE, r
    assert r["failed_share"] <= 0.01, r
    assert r["base_inside"] == 0 and r["min_base_clearance_m"] > 0.0, r
    assert r["min_ee_clearance_m"] >= 0.5 * r["r_body"], r
    b = ex.run(B=256, steps=STEPS, seed=0, lidar=False)
    print(b)
    assert b["min_ee_clearance_m"] < 0.5 * b["r_body"], b
