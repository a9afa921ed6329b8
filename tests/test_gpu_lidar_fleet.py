"""The fleet in the scan on the device (rmpc_lidar_scan_fleet_device) against the numpy restatement of
tests/lidar_fleet_reference.py, bitwise against the plain scan (its static world; brute force with the bodies appended
as circles; the cull's boundary), the refusals of the C ABI, stream and device selection, LidarPlanes with bodies, and the
closed loop of examples/fleet_crossing_lidar.py."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from example_loader import load_example
from gpu_support import DEV, _t
from lidar_fleet_cases import (BODY_OFFSET, DENSE_MIN_IN_RANGE, HEIGHT, OFFSET, PARITY_CASES, RANGE, excluded,
                               fleet_world, in_range_counts, outcome_shares, parity_case, sensor_centred)
from lidar_fleet_reference import fleet_scan_ref

pytestmark = pytest.mark.gpu

FULL = (-math.pi, math.pi)


@pytest.fixture(scope="module")
def rt():
    import torch
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return dict(torch=torch, lib=_lib)


def _fleet(rt, pose, R, boxes, circles, centres, radius, self0=0, sweep=FULL, max_range=RANGE, offset=OFFSET,
           stream=None, dev=DEV):
    """the fleet scan from NaN-filled outputs -> dict of numpy arrays"""
    torch = rt["torch"]
    B = pose.shape[0]
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=dev)
    pts, rng_, srng = nan(B, R, 3), nan(B, R), nan(B, R)
    own = torch.full((B, R), -99, dtype=torch.int32, device=dev)
    world = [None if a is None else _t(torch, a, dev=dev) for a in (boxes, circles)]
    rt["lib"].lidar_scan_fleet_device(_t(torch, pose, dev=dev), pts, _t(torch, centres, dev=dev),
                                      _t(torch, radius, dev=dev), world[0], world[1],
                                      sweep[0], sweep[1], max_range, offset, HEIGHT, self0=self0, owner=own,
                                      static_ranges=srng, ranges=rng_, stream=stream)
    torch.cuda.synchronize(dev)
    return dict(points=pts.cpu().numpy(), ranges=rng_.cpu().numpy(), static_ranges=srng.cpu().numpy(),
                owner=own.cpu().numpy())


def _plain(rt, pose, R, boxes, circles, sweep=FULL, max_range=RANGE, offset=OFFSET):
    torch = rt["torch"]
    B = pose.shape[0]
    pts = torch.full((B, R, 3), float("nan"), dtype=torch.float64, device=DEV)
    rng_ = torch.full((B, R), float("nan"), dtype=torch.float64, device=DEV)
    rt["lib"].lidar_scan_device(_t(torch, pose), pts, _t(torch, boxes), _t(torch, circles), sweep[0], sweep[1],
                                max_range, offset, HEIGHT, ranges=rng_)
    torch.cuda.synchronize()
    return pts.cpu().numpy(), rng_.cpu().numpy()


@pytest.mark.parametrize("n", range(len(PARITY_CASES)))
def test_fleet_scan_matches_restatement(rt, n):
    """(a) the tolerances of test_scan_matches_restatement on the rays kept; the owner is equal on them"""
    c = parity_case(n)
    ref = c["ref"]
    got = _fleet(rt, c["pose"], c["R"], c["boxes"], c["circles"], c["centres"], c["radius"], c["self0"])
    excl = excluded(ref)
    print(PARITY_CASES[n][:4], "excluded", excl.mean(), "outcomes", outcome_shares(ref))
    assert excl.mean() < 0.01, excl.mean()
    assert all(s > 0 for s in outcome_shares(ref)), outcome_shares(ref)
    if n == len(PARITY_CASES) - 1:
        # the dense case: more bodies in range of every robot than the kernel's list holds at once
        assert in_range_counts(c).min() >= DENSE_MIN_IN_RANGE > rt["lib"].LIDAR_FLEET_LIST
    keep = ~excl
    assert np.all(np.isfinite(got["points"])) and np.all(got["points"][:, :, 2] == HEIGHT)
    print("max |dt|", np.abs(got["ranges"] - ref["ranges"])[keep].max(),
          "max |dpoint|", np.abs(got["points"] - ref["points"]).max(axis=2)[keep].max(),
          "max |dts|", np.abs(got["static_ranges"] - ref["static_ranges"])[keep].max(),
          "owner differs on", int((got["owner"] != ref["owner"])[keep].sum()))
    assert np.abs(got["ranges"] - ref["ranges"])[keep].max() <= 1e-12
    assert np.abs(got["points"] - ref["points"]).max(axis=2)[keep].max() <= 1e-12
    assert np.abs(got["static_ranges"] - ref["static_ranges"])[keep].max() <= 1e-12
    assert np.array_equal(got["owner"][keep], ref["owner"][keep])
    assert np.all(got["ranges"] <= got["static_ranges"]) and np.all(got["static_ranges"] <= RANGE)


@pytest.mark.parametrize("n", [1, 2, 4])
def test_static_world_is_bitwise_the_plain_scan(rt, n):
    """(b) device against device on the same rmpc_lidar: static_ranges are the plain scan's ranges; with P = 0 the whole
    result is the plain scan's"""
    c = parity_case(n)
    p_pts, p_rng = _plain(rt, c["pose"], c["R"], c["boxes"], c["circles"])
    got = _fleet(rt, c["pose"], c["R"], c["boxes"], c["circles"], c["centres"], c["radius"], c["self0"])
    assert np.array_equal(got["static_ranges"], p_rng)
    none = _fleet(rt, c["pose"], c["R"], c["boxes"], c["circles"], np.zeros((0, 3)), np.zeros(0), c["self0"])
    assert np.array_equal(none["points"], p_pts) and np.array_equal(none["ranges"], p_rng)
    assert np.array_equal(none["static_ranges"], p_rng)
    assert np.array_equal(none["owner"], np.where(p_rng < RANGE, -2, -1))
    assert (none["owner"] == -2).any() and (none["owner"] == -1).any()


def test_brute_force_at_full_size_is_bitwise(rt):
    """(c) B = P = 4099, R = 64, bodies centred on the sensors: points and ranges equal the plain scan with the bodies
    appended to its circles -- no tolerance, so the cull drops nothing"""
    B, R = 4099, 64
    rng = np.random.default_rng(4099)
    pose, boxes, circles, centres, radius, allc = sensor_centred(rng, B, 72.0)
    got = _fleet(rt, pose, R, boxes, circles, centres, radius, 0, max_range=10.0)
    p_pts, p_rng = _plain(rt, pose, R, boxes, allc, max_range=10.0)
    assert np.array_equal(got["ranges"], p_rng) and np.array_equal(got["points"], p_pts)
    seen = (got["owner"] >= 0).mean()
    print("rays that end on a body", seen)
    assert 0.05 < seen < 0.95 and (got["owner"] == -1).any()
    # owner: the body whose circle gives that distance
    b, i = np.nonzero(got["owner"] >= 0)
    assert np.all(got["owner"][b, i] != b)


def test_cull_boundary(rt):
    """(d) sin / cos exact (heading 0, no offset, one ray at angle 0): one robot per body on its own line y = 100 b,
    the body on that line at range + r -+ delta.  Bitwise equal to the restatement in ranges and owner."""
    rng_, deltas = 9.0, []
    for r in (0.5, 0.3):
        d0 = rng_ + r
        for delta in (0.0, np.nextafter(d0, np.inf) - d0, 1e-12, 1e-9, 1e-3):
            deltas += [(r, d0 - delta), (r, d0 + delta)]
    B = len(deltas)
    pose = np.zeros((B, 3))
    pose[:, 1] = 100.0 * np.arange(B)
    centres = np.stack([np.array([d for _, d in deltas]), pose[:, 1], np.zeros(B)], axis=1)
    radius = np.array([r for r, _ in deltas])
    sweep, off = (0.0, 2.0 * math.pi), (0.0, 0.0)
    ref = fleet_scan_ref(pose, 1, sweep[0], sweep[1], rng_, off, HEIGHT, None, None, centres, radius, B)
    got = _fleet(rt, pose, 1, None, None, centres, radius, B, sweep=sweep, max_range=rng_, offset=off)
    print("ranges", got["ranges"][:, 0].tolist(), "owner", got["owner"][:, 0].tolist())
    assert np.array_equal(got["ranges"], ref["ranges"]) and np.array_equal(got["owner"], ref["owner"])
    # both sides of the boundary are present: bodies seen just inside the range, nothing beyond it
    assert (ref["owner"] >= 0).any() and (ref["owner"] == -1).any()
    assert np.array_equal(got["owner"][got["owner"] >= 0], np.flatnonzero(got["owner"][:, 0] >= 0))


def test_refusals(rt):
    """(e)"""
    torch, lib = rt["torch"], rt["lib"]
    L = lib.load_library()
    B, R, P = 4, 8, 6
    f64 = dict(dtype=torch.float64, device=DEV)
    pose, pts = torch.zeros((B, 8), **f64), torch.zeros((B, R, 3), **f64)
    boxes = torch.tensor([[1.0, 0.0, 0.5, 0.5]], **f64)
    circles = torch.tensor([[0.0, 2.0, 0.5]], **f64)
    centres, radius = torch.zeros((P, 3), **f64), torch.full((P,), 0.3, **f64)
    own = torch.zeros((B, R), dtype=torch.int32, device=DEV)

    def scan(B_=B, fleet=None, **kw):
        a = lib.lidar_args(pose, pts, boxes, circles)
        f = lib.lidar_bodies_args(centres, radius, 0, own)
        for k, v in kw.items():
            setattr(a, k, v)
        for k, v in (fleet or {}).items():
            setattr(f, k, v)
        rc = L.rmpc_lidar_scan_fleet_device(B_, C.byref(a), C.byref(f), None)
        return rc, L.rmpc_last_error().decode()

    assert scan()[0] == 0
    size = C.sizeof(lib.LidarArgs)
    # everything the plain scan refuses
    bad = [dict(struct_size=size + 8), dict(struct_size=size - 8), dict(rays=0), dict(B_=0), dict(pose_stride=2),
           dict(range=0.0), dict(range=-1.0), dict(range=math.inf), dict(range=math.nan), dict(pose=None),
           dict(points=None), dict(boxes=None), dict(circles=None), dict(nbox=-1), dict(ncircle=-1),
           dict(B_=1 << 20, rays=1 << 12), dict(nbox=1 << 30), dict(ncircle=1 << 30)]
    for kw in bad:
        rc, msg = scan(**kw)
        assert rc == -1 and msg, kw
    fsize = C.sizeof(lib.LidarBodiesArgs)
    for fl in (dict(struct_size=fsize + 8), dict(struct_size=fsize - 8), dict(struct_size=0), dict(P=-1),
               dict(centres=None), dict(radius=None), dict(centre_stride=1), dict(centre_stride=0),
               dict(centre_stride=-3), dict(P=1 << 29, centre_stride=8), dict(P=1 << 30, centre_stride=3)):
        rc, msg = scan(fleet=fl)
        assert rc == -1 and msg, fl
    assert L.rmpc_lidar_scan_fleet_device(B, None, None, None) == -1
    a = lib.lidar_args(pose, pts, boxes, circles)
    assert L.rmpc_lidar_scan_fleet_device(B, C.byref(a), None, None) == -1
    # legal: no bodies with NULL arrays, NULL optional outputs, a robot index outside the bodies
    assert scan(fleet=dict(P=0, centres=None, radius=None))[0] == 0
    assert scan(fleet=dict(owner=None, static_ranges=None))[0] == 0
    assert scan(fleet=dict(self0=-7))[0] == 0 and scan(fleet=dict(self0=(1 << 31) - 1))[0] == 0
    torch.cuda.synchronize()


def _planes_chain(rt, lp, pose, z, ef, stream):
    torch = rt["torch"]
    with torch.cuda.stream(stream):
        lp.step(pose, z, ef)
    stream.synchronize()
    return tuple(t.cpu().numpy() for t in (lp.centres, lp.points, lp.ranges, lp.static_ranges, lp.owner, lp.seeds, lp.planes))


def _planes_inputs(rt, dev=DEV):
    torch = rt["torch"]
    B, N, K = 300, 10, 4
    rng = np.random.default_rng(11)
    pose, boxes, circles, _, radius = fleet_world(rng, B, B, 0, 12.0, (0.3, 0.6))
    z = rng.normal(scale=0.1, size=(B, N, 10))
    z[:, :, :3] += pose[:, None, :3]
    ef = rng.choice(np.array([-1, 0, 1], np.int32), B)
    return (B, N, K, boxes, circles, radius), (_t(torch, pose, dev=dev), _t(torch, z, dev=dev),
                                               _t(torch, ef, torch.int32, dev=dev))


def _lidar_planes(cfg, dev=DEV, **kw):
    from robot_mpcs_amd.utils.lidar import LidarPlanes
    B, N, K, boxes, circles, radius = cfg
    return LidarPlanes(B, N, K, boxes=boxes, circles=circles, max_range=RANGE, offset=OFFSET, device=dev, **kw)


def test_stream_ordering(rt):
    """(f) centres -> fleet scan -> seeds -> FSD on a side stream, three times from NaN-filled outputs"""
    torch = rt["torch"]
    cfg, args = _planes_inputs(rt)
    lp = _lidar_planes(cfg, body_radius=cfg[5], body_offset=BODY_OFFSET)
    ref = _planes_chain(rt, lp, *args, torch.cuda.default_stream(0))
    assert (ref[4] >= 0).any() and (ref[4] == -2).any() and (ref[4] == -1).any()
    side = torch.cuda.Stream(device=0)
    for _ in range(3):
        for t in (lp.centres, lp.points, lp.ranges, lp.static_ranges, lp.planes):
            t.fill_(float("nan"))
        lp.owner.fill_(-99)
        got = _planes_chain(rt, lp, *args, side)
        assert all(np.array_equal(a, b) for a, b in zip(ref, got))


def test_device_selection_on_a_second_gpu(rt):
    """(g) the chain on cuda:1 while cuda:0 is current"""
    torch = rt["torch"]
    if torch.cuda.device_count() < 2:
        pytest.skip("device selection: one GPU visible")
    cfg, args = _planes_inputs(rt)
    lp = _lidar_planes(cfg, body_radius=cfg[5], body_offset=BODY_OFFSET)
    ref = _planes_chain(rt, lp, *args, torch.cuda.default_stream(0))
    torch.cuda.set_device(0)
    cfg1, args1 = _planes_inputs(rt, "cuda:1")
    lp1 = _lidar_planes(cfg1, "cuda:1", body_radius=cfg1[5], body_offset=BODY_OFFSET)
    with torch.cuda.device(0):
        lp1.step(*args1)
    torch.cuda.synchronize(1)
    got = tuple(t.cpu().numpy() for t in (lp1.centres, lp1.points, lp1.ranges, lp1.static_ranges, lp1.owner, lp1.seeds,
                                           lp1.planes))
    assert all(np.array_equal(a, b) for a, b in zip(ref, got))


def test_lidar_planes_with_bodies_is_the_four_launches(rt):
    """(h) step with body_radius = fleet points, fleet scan, plan points, FSD made by hand, bit for bit; bodies= handed
    to step likewise; without either it is today's three launches"""
    torch, lib = rt["torch"], rt["lib"]
    cfg, (pose, z, ef) = _planes_inputs(rt)
    B, N, K, boxes, circles, radius = cfg
    f64 = dict(dtype=torch.float64, device=DEV)
    tb, tc, tr = _t(torch, boxes), _t(torch, circles), _t(torch, radius)

    def by_hand(bodies):
        pts, rng_, srng = torch.zeros((B, 64, 3), **f64), torch.zeros((B, 64), **f64), torch.zeros((B, 64), **f64)
        own = torch.zeros((B, 64), dtype=torch.int32, device=DEV)
        seeds, planes = torch.zeros((B, N, 3), **f64), torch.zeros((B, N, K, 4), **f64)
        if bodies == "own":
            cen = torch.zeros((B, 1, 3), **f64)
            lib.fleet_points_device(pose, cen, None, None, 1, BODY_OFFSET, 0.0)
            bodies = (cen, tr, 0)
        if bodies is None:
            lib.lidar_scan_device(pose, pts, tb, tc, -math.pi, math.pi, RANGE, OFFSET, 0.02, ranges=rng_)
        else:
            lib.lidar_scan_fleet_device(pose, pts, bodies[0], bodies[1], tb, tc, -math.pi, math.pi, RANGE, OFFSET, 0.02,
                                        self0=bodies[2], owner=own, static_ranges=srng, ranges=rng_)
        lib.plan_points_device(pose, seeds, z, ef, OFFSET, 0.02)
        lib.free_space_decomposition_device(pts, seeds, planes, 5.0)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (pts, rng_, srng, own, seeds, planes)]

    def of(lp):
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (lp.points, lp.ranges, lp.static_ranges, lp.owner, lp.seeds, lp.planes)]

    lp = _lidar_planes(cfg, body_radius=radius, body_offset=BODY_OFFSET)
    assert lp.step(pose, z, ef) is lp.planes
    hand = by_hand("own")
    assert all(np.array_equal(a, b) for a, b in zip(hand, of(lp)))
    assert (hand[3] >= 0).mean() > 0.02
    # a scalar radius, the default body offset (the sensor's): bodies centred on the sensors
    lp_s = _lidar_planes(cfg, body_radius=0.45)
    lp_s.step(pose, z, ef)
    cen = torch.zeros((B, 1, 3), **f64)
    lib.fleet_points_device(pose, cen, None, None, 1, OFFSET, 0.0)
    others = (cen, torch.full((B,), 0.45, **f64), 0)
    assert all(np.array_equal(a, b) for a, b in zip(by_hand(others), of(lp_s)))
    # bodies handed to step: other blocks' robots (here 40 of the same, so robot b is body b - 7 or none)
    part = (cen[7:47].contiguous(), tr[7:47].contiguous(), -7)
    lp_b = _lidar_planes(cfg)
    lp_b.step(pose, z, ef, bodies=part)
    assert all(np.array_equal(a, b) for a, b in zip(by_hand(part), of(lp_b)))
    # without either argument: the plain scan, no fleet buffers
    lp_0 = _lidar_planes(cfg)
    lp_0.step(pose, z, ef)
    assert lp_0.owner is None and lp_0.static_ranges is None and lp_0.centres is None
    torch.cuda.synchronize()
    h0 = by_hand(None)
    got0 = [t.cpu().numpy() for t in (lp_0.points, lp_0.ranges, lp_0.seeds, lp_0.planes)]
    assert all(np.array_equal(a, b) for a, b in zip([h0[0], h0[1], h0[4], h0[5]], got0))
    # and the bodies change what the solver is told
    assert not np.array_equal(h0[5], hand[5])


LOOP_STEPS = 200     # twice the blind fleet's last arrival (step 97): every crossing has happened


@pytest.fixture(scope="module")
def blind_loop(rt):
    r = load_example("fleet_crossing_lidar").run("blind", B=64, steps=LOOP_STEPS, seed=0)
    print(json.dumps(r))
    return r


@pytest.mark.parametrize("mode", ["seen", "tracked"])
def test_closed_loop_robots_that_see_each_other_keep_apart(rt, blind_loop, mode):
    """(i) 64 boxers cross the open floor (examples/fleet_crossing_lidar.py, seed 0, 200 control steps) with nothing
    but their own scans.  The gate is relative to the blind run of the same module: blind has pair-steps below
    r_i + r_j (otherwise the comparison says nothing); seen and tracked each have strictly fewer and a larger least
    ratio of distance to r_i + r_j; all three run on the fused kernel.  First MI355X measurement over 400 steps
    (DESIGN.md 20), pair-steps / least ratio / failed share: blind 2355 / 0.021 / 0.004 %, seen 68 / 0.836 / 17.5 %,
    tracked 219 / 0.157 / 0.15 %; the lines of this test's 200 steps are tests/golden/seen_loops.json.  The
    failed-solve share of each mode is printed as it comes out."""
    blind = blind_loop
    r = load_example("fleet_crossing_lidar").run(mode, B=64, steps=LOOP_STEPS, seed=0)
    print(json.dumps(r))
    print("failed share: blind", blind["failed_share"], mode, r["failed_share"])
    assert blind["fused"] and r["fused"]
    assert blind["below_pair_steps"] > 0, blind
    assert r["below_pair_steps"] < blind["below_pair_steps"], (r, blind)
    assert r["min_ratio"] > blind["min_ratio"], (r, blind)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seen_loops.json")) as f:
        golden = json.load(f)
    assert set(golden) == {"blind", "seen", "tracked"} and golden[mode]["steps"] == LOOP_STEPS
