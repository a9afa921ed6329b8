"""Fleet separation's rules (include/rmpc.h, rmpc_fleet_points_device / rmpc_fleet_planes_device)
as restated in tests/fleet_planes_reference.py, checked on hand-computed cases, the guarantee of a mutual pair's planes
checked by sampling, and the refusals of both entries through the loaded library (no device needed: arguments are
checked before any HIP call).  tests/test_gpu_fleet_planes.py holds the device against the restatement."""
import ctypes as C
import math

import numpy as np
import pytest

from fleet_planes_reference import dummy_plane, fleet_planes_ref, fleet_points_ref, neighbours_ref


def _dist(plane, p):
    return plane[:3] @ p + plane[3]


def test_two_robots_unequal_radii():
    # 2 m apart along x, radii 0.3 and 0.5: free gap 1.2, the plane at x = 0.3 + 0.6 = 0.9 from robot 0
    pts = np.array([[[0.0, 0.0, 0.0]], [[2.0, 0.0, 0.0]]])
    out = fleet_planes_ref(pts, np.array([0.3, 0.5]), 1, math.inf)
    assert np.array_equal(out[0, 0, 0, :3], [-1.0, 0.0, 0.0]) and out[0, 0, 0, 3] == pytest.approx(0.9, abs=1e-15)
    assert np.array_equal(out[1, 0, 0], -out[0, 0, 0])
    # each point lies r_own + g / 2 from the plane
    assert _dist(out[0, 0, 0], pts[0, 0]) == pytest.approx(0.9, abs=1e-15)
    assert _dist(out[1, 0, 0], pts[1, 0]) == pytest.approx(1.1, abs=1e-15)
    # a diagonal pair: the plane is the perpendicular bisector shifted by the radii
    pts = np.array([[[3.0, 4.0, 0.0]], [[0.0, 0.0, 0.0]]])
    out = fleet_planes_ref(pts, np.array([1.0, 0.5]), 1, math.inf)
    n = np.array([0.6, 0.8, 0.0])
    assert out[0, 0, 0, :3] == pytest.approx(n, abs=1e-15)
    assert _dist(out[0, 0, 0], pts[0, 0]) == pytest.approx(1.0 + 1.75, abs=1e-15)
    assert _dist(out[1, 0, 0], pts[1, 0]) == pytest.approx(0.5 + 1.75, abs=1e-15)
    # overlapping robots: a negative gap, still split equally
    pts = np.array([[[0.0, 0.0, 0.0]], [[0.5, 0.0, 0.0]]])
    out = fleet_planes_ref(pts, np.array([0.3, 0.3]), 1, math.inf)
    assert _dist(out[0, 0, 0], pts[0, 0]) == pytest.approx(0.25, abs=1e-15)
    assert _dist(out[1, 0, 0], pts[1, 0]) == pytest.approx(0.25, abs=1e-15)


def test_ties_go_to_the_lower_index():
    # robots 1, 2, 3, 4 all 1 m from robot 0; K = 2 picks 1 and 2 in that order, whatever the storage order
    pts = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [-1.0, 0.0, 0.0]])[:, None]
    sel = neighbours_ref(pts, 2, math.inf)
    assert sel[0, 0].tolist() == [1, 2]
    # robot 2: robot 0 at 1, robots 1 and 3 at sqrt 2 -> 0, 1
    assert sel[2, 0].tolist() == [0, 1]
    out = fleet_planes_ref(pts, np.full(5, 0.2), 2, math.inf)
    assert np.array_equal(out[0, 0, 0], -out[1, 0, 0]) and np.array_equal(out[0, 0, 1], -out[2, 0, 0])


def test_coincident_points():
    pts = np.array([[[1.0, 2.0, 0.0]], [[1.0, 2.0, 0.0]]])
    out = fleet_planes_ref(pts, np.array([0.3, 0.4]), 1, math.inf)
    # n = (1, 0, 0), g = -0.7, m = q_hi + (0.4 - 0.35) n = (1.05, 2, 0), c = -1.05
    assert np.array_equal(out[0, 0, 0, :3], [1.0, 0.0, 0.0]) and out[0, 0, 0, 3] == pytest.approx(-1.05, abs=1e-15)
    assert np.array_equal(out[1, 0, 0], -out[0, 0, 0])


def test_range_is_exclusive():
    pts = np.array([[[0.0, 0.0, 0.0]], [[3.0, 0.0, 0.0]], [[0.0, 2.5, 0.0]]])
    sel = neighbours_ref(pts, 2, 3.0)
    assert sel[0, 0].tolist() == [2, -1]          # robot 1 sits exactly at the range: not admitted
    assert neighbours_ref(pts, 2, 0.0).max() == -1
    assert neighbours_ref(pts, 2, math.inf)[0, 0].tolist() == [2, 1]


def test_k_above_the_candidates_gives_dummy_planes():
    pts = np.array([[[0.0, 0.0, 0.1]], [[1.0, 0.0, 0.1]]])
    sentinel = np.full((2, 1, 6, 4), 7.0)
    out = fleet_planes_ref(pts, np.array([0.3, 0.3]), 4, math.inf, nobst=6, slot0=1, planes=sentinel)
    assert np.array_equal(out[0, 0, 2], [-20.0, -20.0, 0.0, 800.0])
    assert np.array_equal(out[0, 0, 2], dummy_plane(pts[0, 0]))
    assert np.array_equal(out[1, 0, 3], dummy_plane(pts[1, 0])) and np.array_equal(out[1, 0, 4], dummy_plane(pts[1, 0]))
    # slots outside [slot0, slot0 + K) are untouched
    assert np.all(out[:, :, 0] == 7.0) and np.all(out[:, :, 5] == 7.0)
    # the dummy plane keeps its seed 20 sqrt 2 away: inactive for any robot near its seed
    assert _dist(dummy_plane(pts[0, 0]), pts[0, 0]) / np.linalg.norm(dummy_plane(pts[0, 0])[:3]) == \
        pytest.approx(20 * math.sqrt(2), rel=1e-15)


def test_points_shift_and_held_last_stage():
    pose = np.array([[9.0, 9.0, 0.0, 0, 0, 0]])
    N, nvar = 4, 6
    z = np.zeros((1, N, nvar))
    z[0, :, 0] = [10.0, 11.0, 12.0, 13.0]
    z[0, :, 2] = [0.0, math.pi / 2, 0.0, math.pi]
    p = fleet_points_ref(pose, N, z, np.array([1], np.int32), heading=0, height=0.05)
    assert p[0, :, 0].tolist() == [11.0, 12.0, 13.0, 13.0] and np.all(p[0, :, 2] == 0.05)
    p = fleet_points_ref(pose, N, z, None, heading=1, offset=(0.4, 0.0))
    assert p[0, :, :2] == pytest.approx(np.array([[11.0, 0.4], [12.4, 0.0], [12.6, 0.0], [12.6, 0.0]]), abs=1e-15)
    # N = 1: the only stage is held
    assert fleet_points_ref(pose, 1, z[:, :1], heading=0)[0, 0, 0] == 10.0


def test_points_failed_solve_and_first_step():
    pose = np.array([[1.0, 2.0, math.pi / 2, 0, 0], [-3.0, 0.5, 0.0, 0, 0]])
    z = np.ones((2, 3, 5)) * 4.0
    first = fleet_points_ref(pose, 3, None, heading=1)
    assert first[0] == pytest.approx(np.array([[1.0, 2.4, 0.0]] * 3), abs=1e-15)
    f = fleet_points_ref(pose, 3, z, np.array([-7, 2], np.int32), heading=1)
    assert np.array_equal(f[0], first[0]) and not np.array_equal(f[1], first[1])
    f0 = fleet_points_ref(pose, 3, z, np.array([0, -1], np.int32), heading=0, height=0.05)
    assert f0[0].tolist() == [[4.0, 4.0, 0.05]] * 3 and f0[1].tolist() == [[-3.0, 0.5, 0.05]] * 3


def test_mutual_planes_separate_points_on_their_own_sides():
    """Any two points that lie on their own sides of a mutual pair's planes, at least r_own from them, are at least
    r_i + r_j apart: sampled over random pairs (overlapping predictions included) and random points."""
    rng = np.random.default_rng(0)
    worst = math.inf
    for _ in range(300):
        pts = rng.uniform(-1.5, 1.5, (2, 1, 3))
        pts[:, :, 2] *= rng.integers(0, 2)            # planar or 3-D
        r = rng.uniform(0.1, 0.8, 2)
        out = fleet_planes_ref(pts, r, 1, math.inf)
        assert np.array_equal(out[0, 0, 0], -out[1, 0, 0])
        sample = rng.uniform(-4, 4, (4000, 2, 3))
        ok0 = sample[:, 0] @ out[0, 0, 0, :3] + out[0, 0, 0, 3] >= r[0]
        ok1 = sample[:, 1] @ out[1, 0, 0, :3] + out[1, 0, 0, 3] >= r[1]
        keep = ok0 & ok1
        assert keep.any()
        d = np.linalg.norm(sample[keep, 0] - sample[keep, 1], axis=1)
        worst = min(worst, float((d - r.sum()).min()))
    assert worst >= -1e-12


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return _lib


def test_refusals(lib):
    """Every refusal of both entries, before any HIP call: each returns -1 with the entry's own message (never the HIP
    runtime's, which a call that passed validation would report on a machine without a device).  Host-side fake
    pointers are never dereferenced; tests/test_gpu_fleet_planes.py shows the same valid calls return 0 on a device."""
    L = lib.load_library()
    P = C.c_void_p(0x1000)

    def planes(B=4, N=3, pts=P, rad=P, K=2, rng=1.0, nobst=4, slot0=0, out=P):
        rc = L.rmpc_fleet_planes_device(B, N, pts, rad, K, rng, nobst, slot0, out, None)
        return rc, L.rmpc_last_error().decode()

    cases = [(dict(pts=None), "null argument"), (dict(rad=None), "null argument"), (dict(out=None), "null argument"),
             (dict(B=0), "need B, N >= 1"), (dict(N=0), "need B, N >= 1"), (dict(K=0), "1 <= K <= 8"),
             (dict(K=9, nobst=9), "1 <= K <= 8"), (dict(slot0=-1), "slot0 + K <= nobst"),
             (dict(slot0=3), "slot0 + K <= nobst"), (dict(K=5), "slot0 + K <= nobst"),
             (dict(nobst=0), "slot0 + K <= nobst"), (dict(rng=-1.0), "range must be >= 0"),
             (dict(rng=math.nan), "range must be >= 0"), (dict(rng=-math.inf), "range must be >= 0"),
             (dict(B=1 << 16, N=1 << 10, nobst=8), "INT_MAX"), (dict(B=1 << 14, N=1 << 14, nobst=8, K=8), "INT_MAX")]
    for kw, want in cases:
        rc, msg = planes(**kw)
        assert rc == -1 and want in msg and "hip" not in msg.lower(), (kw, msg)

    def points(B=4, N=3, z=P, nvar=10, ef=None, pose=P, stride=8, heading=1, out=P):
        rc = L.rmpc_fleet_points_device(B, N, z, nvar, ef, pose, stride, heading, 0.4, 0.0, 0.0, out, None)
        return rc, L.rmpc_last_error().decode()

    cases = [(dict(pose=None), "null argument"), (dict(out=None), "null argument"), (dict(B=0), "need B, N >= 1"),
             (dict(N=0), "need B, N >= 1"), (dict(heading=2), "heading must be 0 or 1"),
             (dict(heading=-1), "heading must be 0 or 1"), (dict(nvar=2), "nvar must be >= 3"),
             (dict(stride=2), "pose_stride must be >= 3"), (dict(B=1 << 16, N=1 << 16), "INT_MAX"),
             (dict(B=1 << 12, N=1 << 10, nvar=1 << 10), "INT_MAX"), (dict(B=1 << 29, stride=8), "INT_MAX")]
    for kw, want in cases:
        rc, msg = points(**kw)
        assert rc == -1 and want in msg and "hip" not in msg.lower(), (kw, msg)
