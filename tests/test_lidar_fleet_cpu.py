"""The fleet scan's rule (include/rmpc.h, rmpc_lidar_bodies) as restated in tests/lidar_fleet_reference.py,
checked on hand-computed cases; tests/test_gpu_lidar_fleet.py holds the device against the restatement.  Also the
refusals of the C ABI that need no device, and the shares of the parity cases' rays that the device test sets aside."""
import ctypes as C
import math

import numpy as np
import pytest

from lidar_fleet_cases import (DENSE_MIN_IN_RANGE, PARITY_CASES, excluded, in_range_counts, outcome_shares, parity_case,
                               sensor_centred)
from lidar_fleet_reference import fleet_scan_ref
from lidar_reference import scan_ref


def one_ray(pose, angle, centres, radius, boxes=None, circles=None, self0=0, max_range=10.0, offset=(0.0, 0.0)):
    """The single ray at `angle` of every robot in `pose`: (ranges (B,), owner (B,), static_ranges (B,))."""
    r = fleet_scan_ref(np.atleast_2d(np.asarray(pose, dtype=float)), 1, angle, angle + 2 * math.pi, max_range, offset,
                       0.02, boxes, circles, centres, radius, self0)
    return r["ranges"][:, 0], r["owner"][:, 0], r["static_ranges"][:, 0]


def test_exact_hit():
    # u = (-3, 0), bb = -3, cc = 9 - 0.25, disc = 9 - 8.75 = 0.25, t = 3 - 0.5
    t, own, ts = one_ray((0.0, 0.0, 0.0), 0.0, [(3.0, 0.0)], [0.5], self0=7)
    assert t[0] == 2.5 and own[0] == 0 and ts[0] == 10.0
    r = fleet_scan_ref(np.zeros((1, 3)), 1, 0.0, 2 * math.pi, 10.0, (0.0, 0.0), 0.02, None, None, [(3.0, 0.0)], [0.5], 7)
    assert np.array_equal(r["points"][0, 0], [2.5, 0.0, 0.02])


def test_own_body_is_never_seen():
    # the robot's own body 1 m ahead of the sensor: the ray passes through it and ends on the other robot's body
    pose = [(0.0, 0.0, 0.0), (5.0, 0.0, 0.0)]
    centres, radius = [(1.0, 0.0), (6.0, 0.0)], [0.25, 0.25]
    t, own, _ = one_ray(pose, 0.0, centres, radius)
    assert t[0] == 5.75 and own[0] == 1          # robot 0 does not see body 0
    assert t[1] == 10.0 and own[1] == -1         # robot 1 does not see body 1, body 0 lies behind it
    # the same bodies as somebody else's (self0 moves the robots off them): both are seen
    t, own, _ = one_ray(pose, 0.0, centres, radius, self0=2)
    assert t[0] == 0.75 and own[0] == 0 and t[1] == 0.75 and own[1] == 1


def test_occlusion_and_ties():
    body, rad = [(6.0, 0.0)], [1.0]                                   # hit at 5
    t, own, ts = one_ray((0.0, 0.0, 0.0), 0.0, body, rad, boxes=[(3.0, 0.0, 2.0, 2.0)], self0=5)
    assert t[0] == 2.0 and own[0] == -2 and ts[0] == 2.0              # a box in front of the body
    t, own, ts = one_ray((0.0, 0.0, 0.0), 0.0, body, rad, boxes=[(8.0, 0.0, 2.0, 2.0)], self0=5)
    assert t[0] == 5.0 and own[0] == 0 and ts[0] == 7.0               # the body in front of a box
    t, own, ts = one_ray((0.0, 0.0, 0.0), 0.0, body, rad, boxes=[(6.0, 0.0, 2.0, 2.0)], self0=5)
    assert t[0] == 5.0 and own[0] == -2 and ts[0] == 5.0              # equal distances: the static world wins
    t, own, ts = one_ray((0.0, 0.0, 0.0), 0.0, body, rad, circles=[(6.0, 0.0, 1.0)], self0=5)
    assert t[0] == 5.0 and own[0] == -2
    # two equal bodies: the lower j wins, whichever comes first
    for centres in ([(9.0, 9.0), (6.0, 0.0), (6.0, 0.0)], [(6.0, 0.0), (9.0, 9.0), (6.0, 0.0)]):
        t, own, _ = one_ray((0.0, 0.0, 0.0), 0.0, centres, [1.0, 1.0, 1.0], self0=5)
        assert t[0] == 5.0 and own[0] == (1 if centres[0] == (9.0, 9.0) else 0)
    # a nearer body with a higher index still wins over a farther one with a lower index
    t, own, _ = one_ray((0.0, 0.0, 0.0), 0.0, [(6.0, 0.0), (4.0, 0.0)], [1.0, 1.0], self0=5)
    assert t[0] == 3.0 and own[0] == 1


def test_radius_not_positive_or_nan_is_skipped():
    centres = [(2.0, 0.0), (3.0, 0.0), (4.0, 0.0), (6.0, 0.0)]
    t, own, _ = one_ray((0.0, 0.0, 0.0), 0.0, centres, [0.0, -0.5, math.nan, 1.0], self0=9)
    assert t[0] == 5.0 and own[0] == 3
    # a NaN centre never hits either
    t, own, _ = one_ray((0.0, 0.0, 0.0), 0.0, [(math.nan, 0.0), (2.0, math.nan), (6.0, 0.0)], [1.0, 1.0, 1.0], self0=9)
    assert t[0] == 5.0 and own[0] == 2


def test_origin_inside_a_foreign_body():
    # the sensor of robot 0 lies inside body 1 (and on the rim of body 2): both are ignored in every direction
    centres, radius = [(50.0, 50.0), (0.2, 0.1), (1.0, 0.0), (6.0, 0.0)], [0.3, 1.0, 1.0, 1.0]
    r = fleet_scan_ref(np.zeros((1, 3)), 16, -math.pi, math.pi, 10.0, (0.0, 0.0), 0.02, None, None, centres, radius, 0)
    assert set(np.unique(r["owner"])) == {-1, 3}
    assert r["ranges"][0, 8] == 5.0 and r["owner"][0, 8] == 3        # ray 8 of 16 from -pi: the angle 0


def test_self0_with_more_bodies_than_robots():
    # bodies 0 .. 4 stand on the x axis at 2 j + 2; the two robots are bodies 2 and 3 and look along +x from x = 0, 1
    centres = [(2.0 * j + 2.0, 5.0 if j in (2, 3) else 0.0) for j in range(5)]
    pose = [(0.0, 5.0, 0.0), (1.0, 5.0, 0.0)]
    t, own, _ = one_ray(pose, 0.0, centres, [0.5] * 5, self0=2, max_range=20.0)
    assert t[0] == 7.5 and own[0] == 3          # robot 0 is body 2 (at x = 6): it looks through it and sees body 3 at 8
    assert t[1] == 4.5 and own[1] == 2          # robot 1 is body 3: it sees body 2
    # a robot outside [0, P) has no body of its own
    t, own, _ = one_ray(pose, 0.0, centres, [0.5] * 5, self0=4, max_range=20.0)
    assert t[0] == 5.5 and own[0] == 2 and t[1] == 4.5 and own[1] == 2
    t, own, _ = one_ray(pose, 0.0, centres, [0.5] * 5, self0=-3, max_range=20.0)
    assert own[0] == 2 and own[1] == 2


def test_no_bodies_equals_the_plain_scan():
    rng = np.random.default_rng(1)
    pose, boxes, circles, *_ = sensor_centred(rng, 23, 6.0)
    p, t, _ = scan_ref(pose, 33, -math.pi, math.pi, 9.0, (0.4, 0.15), 0.02, boxes, circles)
    r = fleet_scan_ref(pose, 33, -math.pi, math.pi, 9.0, (0.4, 0.15), 0.02, boxes, circles, np.zeros((0, 3)), np.zeros(0))
    assert np.array_equal(r["points"], p) and np.array_equal(r["ranges"], t) and np.array_equal(r["static_ranges"], t)
    assert np.array_equal(r["owner"], np.where(t < 9.0, -2, -1))


def test_owner_codes():
    # three rays of one sweep from heading 0: -pi hits the box, -pi / 3 nothing, pi / 3 ... the body stands on ray 2
    a = math.pi / 3
    centres, radius = [(4.0 * math.cos(a), 4.0 * math.sin(a))], [0.5]
    r = fleet_scan_ref(np.zeros((1, 3)), 3, -math.pi, math.pi, 10.0, (0.0, 0.0), 0.02, [(-5.0, 0.0, 2.0, 2.0)], None,
                       centres, radius, 3)
    assert r["owner"].tolist() == [[-2, -1, 0]] and r["owner"].dtype == np.int32
    assert r["ranges"][0, 0] == pytest.approx(4.0, abs=1e-12) and r["ranges"][0, 1] == 10.0
    assert r["ranges"][0, 2] == pytest.approx(3.5, abs=1e-12)
    assert np.array_equal(r["static_ranges"][0, 1:], [10.0, 10.0])


@pytest.mark.parametrize("B,R,arena", [(41, 64, 6.0), (130, 17, 4.0)])
def test_brute_force_equivalence(B, R, arena):
    """bodies centred on the sensors: the plain scan with the bodies appended to its circles gives the same ranges and
    points bit for bit (a robot's own circle contains its sensor, so the plain rule ignores it as self0 does)"""
    rng = np.random.default_rng(B)
    pose, boxes, circles, centres, radius, allc = sensor_centred(rng, B, arena)
    r = fleet_scan_ref(pose, R, -math.pi, math.pi, 9.0, (0.4, 0.15), 0.02, boxes, circles, centres, radius, 0)
    p, t, _ = scan_ref(pose, R, -math.pi, math.pi, 9.0, (0.4, 0.15), 0.02, boxes, allc)
    assert np.array_equal(r["ranges"], t) and np.array_equal(r["points"], p)
    assert (r["owner"] >= 0).mean() > 0.05


@pytest.mark.parametrize("n", range(len(PARITY_CASES)))
def test_parity_cases_hold_every_outcome(n):
    """what the device test relies on, checked where it is cheap: few rays set aside, all three outcomes present, and
    the dense case fills the kernel's list more than once"""
    from robot_mpcs_amd import _lib
    c = parity_case(n)
    share = excluded(c["ref"]).mean()
    print(PARITY_CASES[n][:4], "excluded", share, "body / occluded body / miss", outcome_shares(c["ref"]))
    assert share < 0.01
    assert all(s > 0 for s in outcome_shares(c["ref"]))
    if n == len(PARITY_CASES) - 1:
        assert in_range_counts(c).min() >= DENSE_MIN_IN_RANGE > _lib.LIDAR_FLEET_LIST


def test_abi_refuses_null_arguments_without_a_gpu():
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    L = _lib.load_library()
    a, f = _lib.LidarArgs(), _lib.LidarBodiesArgs()
    a.struct_size, f.struct_size = C.sizeof(_lib.LidarArgs), C.sizeof(_lib.LidarBodiesArgs)
    for la, lf in ((None, None), (C.byref(a), None), (None, C.byref(f))):
        assert L.rmpc_lidar_scan_fleet_device(4, la, lf, None) == -1
        assert b"null" in L.rmpc_last_error()
    # all pointers NULL in both structs: refused before any device is asked for
    a.rays, a.pose_stride, a.range = 8, 3, 9.0
    assert L.rmpc_lidar_scan_fleet_device(4, C.byref(a), C.byref(f), None) == -1 and b"null" in L.rmpc_last_error()
    f.struct_size += 8
    assert L.rmpc_lidar_scan_fleet_device(4, C.byref(a), C.byref(f), None) == -1
    assert b"rmpc_lidar_bodies" in L.rmpc_last_error()
