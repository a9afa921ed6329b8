"""Constructed calls of the moving-obstacle tracker, one robot each, shared by tests/test_tracking_cpu.py (which pins
the restatement's answer on each by hand) and tests/test_gpu_tracking.py (which holds the device to the restatement on
each).  A case is a dict: points (1, R, 3), ranges (1, R), static (1, R) or None, origin (1, 3), p (the scalars), track
(1, T, 4), age, miss (1, T) int32, n_out."""
import math

import numpy as np

from tracking_reference import detect, params

FAR = 10.0            # the range of every case: a ray of this length is not moving when there is no static scan


def arc(c, o, r, n, half=0.6):
    """n points on the circle (c, r), on the side that faces o, spread over +- half rad"""
    a0 = math.atan2(o[1] - c[1], o[0] - c[0])
    a = a0 + np.linspace(-half, half, n) if n > 1 else np.array([a0])
    return np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a)], axis=1)


def world(R, groups, o=(0.0, 0.0)):
    """points (1, R, 3) and ranges (1, R): the rays of ``groups`` = [(first ray, (n, 2) points)] (around the seam when
    they pass R) are hits at their points, every other ray ends at the range, 8 m out and far from its neighbours"""
    ang = 2.0 * math.pi * np.arange(R) / R
    pts = np.stack([o[0] + 8.0 * np.cos(ang), o[1] + 8.0 * np.sin(ang), np.full(R, 0.02)], axis=1)
    rng = np.full(R, FAR)
    for first, g in groups:
        for t, q in enumerate(np.asarray(g, dtype=float)):
            i = (first + t) % R
            pts[i, :2] = q
            rng[i] = math.hypot(q[0] - o[0], q[1] - o[1])
    return pts[None], rng[None]


def call(points, ranges, T=4, n_out=3, static=None, o=(0.0, 0.0), track=None, age=None, miss=None, **kw):
    c = dict(points=np.ascontiguousarray(points, dtype=float), ranges=np.ascontiguousarray(ranges, dtype=float),
             static=None if static is None else np.ascontiguousarray(static, dtype=float),
             origin=np.array([[o[0], o[1], 0.02]]), p=params(range=FAR, **kw), n_out=n_out,
             track=np.zeros((1, T, 4)), age=np.zeros((1, T), np.int32), miss=np.zeros((1, T), np.int32))
    if track is not None:
        c["track"][0, :len(track)] = track
    if age is not None:
        c["age"][0, :len(age)] = age
    if miss is not None:
        c["miss"][0, :len(miss)] = miss
    return c


def dets_of(c):
    """the detections the restatement finds in a case (to place tracks relative to them)"""
    return detect(c["points"][0, :, :2], c["ranges"][0], None if c["static"] is None else c["static"][0],
                  (c["origin"][0, 0], c["origin"][0, 1]), c["p"])[0]


def line(x0, y, n, dx):
    return np.stack([x0 + dx * np.arange(n), np.full(n, y)], axis=1)


def seam(closed):
    # rays 6, 7, 0, 1 of 8 see one obstacle
    pts, rng = world(8, [(6, arc((3.0, 0.0), (0, 0), 0.3, 4))])
    return call(pts, rng, closed=closed, gap=0.3)


def ring(closed):
    # every ray of 6 is moving and links to its predecessor: a wall of returns all around the sensor
    a = 2.0 * math.pi * np.arange(6) / 6
    pts, rng = world(6, [(0, np.stack([0.25 * np.cos(a), 0.25 * np.sin(a)], axis=1))], o=(0.05, 0.02))
    return call(pts, rng, o=(0.05, 0.02), closed=closed, gap=0.3, max_extent=0.0)


def gap_edge(beyond):
    # two rays 0.5 apart (0.25 = gap^2 exactly), or one ulp more
    x1 = np.nextafter(2.5, 3.0) if beyond else 2.5
    pts, rng = world(8, [(2, [(2.0, 1.0), (x1, 1.0)])])
    return call(pts, rng, gap=0.5, min_rays=1)


def static_edge(below):
    # static 2.0, margin 0.5: a range of exactly 1.5 is not moving, the double below it is
    pts, rng = world(8, [(3, [(1.5, 0.0), (1.5, 0.1)])])
    st = np.full((1, 8), 2.0)
    rng[0, :] = 2.0
    rng[0, 3] = rng[0, 4] = np.nextafter(1.5, 0.0) if below else 1.5
    return call(pts, rng, static=st, margin=0.5, min_rays=1)


def many_segments(n, first_single=False, second_wide=False):
    """n segments of 3 rays each on 4 n rays, 0.6 m apart on a line 3 m ahead; optionally the first a single ray and
    the second 0.5 m wide"""
    groups = []
    for s in range(n):
        g = line(-4.0 + 0.6 * s, 3.0, 3, 0.05)
        if s == 0 and first_single:
            g = g[:1]
        if s == 1 and second_wide:
            g = line(-4.0 + 0.6 * s, 3.2, 3, 0.25)
        groups.append((4 * s, g))
    pts, rng = world(4 * n, groups)
    return call(pts, rng, T=16, n_out=20, gap=0.3, min_rays=2, max_extent=0.45, confirm=1)


def tie_jk():
    # tracks 1 and 2 at the same distance of detection 0; track 0 at the same distance of detections 1 and 2, whose
    # points are mirror images in x taken in the same order, so that their centres are mirror images to the last bit
    A = arc((-0.4, 3.0), (0, 0), 0.3, 3)
    c = call(*world(32, [(2, arc((3.0, 1.2), (0, 0), 0.3, 3)), (10, A), (14, A * np.array([-1.0, 1.0]))]), T=4, gate=1.0,
             confirm=1)
    z = dets_of(c)
    d = 2.0 ** -6
    c["track"][0, 1, :2] = (z[0, 0], z[0, 1] + d)
    c["track"][0, 2, :2] = (z[0, 0], z[0, 1] - d)
    c["track"][0, 0, :2] = (0.0, 3.3)
    c["age"][0, :3] = 2
    return c


def gate_edge(beyond):
    c = call(*world(16, [(2, arc((3.0, 1.2), (0, 0), 0.3, 3))]), T=2, gate=0.5, confirm=1)
    z = dets_of(c)
    c["track"][0, 0, :2] = (z[0, 0], (z[0, 1] + 0.5) if not beyond else np.nextafter(z[0, 1] + 0.5, 9.0))
    c["age"][0, 0] = 4
    return c


def births():
    # slot 0 coasts out in this call, slot 1 is matched, slot 2 is free, slot 3 coasts on: two new detections
    c = call(*world(32, [(2, arc((3.0, 0.0), (0, 0), 0.3, 3)), (10, arc((0.0, 3.0), (0, 0), 0.3, 3)),
                         (20, arc((-3.0, 0.0), (0, 0), 0.3, 3))]), T=4, gate=0.5, confirm=2, max_miss=2)
    z = dets_of(c)
    c["track"][0, 0] = (6.0, 6.0, 0.1, 0.0)
    c["track"][0, 1] = (z[1, 0] + 0.05, z[1, 1], 0.0, -0.2)
    c["track"][0, 3] = (-6.0, 6.0, 0.0, 0.0)
    c["age"][0] = (5, 2, 0, 7)
    c["miss"][0] = (2, 1, 0, 0)
    return c


def full_slots():
    # both slots hold far tracks: the two detections find no slot
    c = call(*world(32, [(2, arc((3.0, 0.0), (0, 0), 0.3, 3)), (10, arc((0.0, 3.0), (0, 0), 0.3, 3))]), T=2, gate=0.5)
    c["track"][0, 0] = (6.0, 6.0, 0.0, 0.0)
    c["track"][0, 1] = (-6.0, 6.0, 0.0, 0.0)
    c["age"][0] = (3, 3)
    return c


def deletion():
    # nothing is seen; miss 1 -> 2 stays (max_miss 2), miss 2 -> 3 goes
    c = call(*world(16, []), T=2, max_miss=2, confirm=1)
    c["track"][0, 0] = (1.0, 1.0, 1.0, -1.0)
    c["track"][0, 1] = (2.0, 2.0, 0.0, 0.0)
    c["age"][0] = (4, 4)
    c["miss"][0] = (1, 2)
    return c


def clamp():
    # the residual of 0.4 m gives v = 0 + 0.5 * 0.4 / 0.1 = 2 > v_max
    c = call(*world(16, [(2, arc((3.0, 0.0), (0, 0), 0.3, 3))]), T=1, gate=1.0, beta=0.5, v_max=0.75, confirm=1)
    z = dets_of(c)
    c["track"][0, 0] = (z[0, 0] - 0.4, z[0, 1] + 0.4, 0.0, 0.0)
    c["age"][0, 0] = 1
    return c


def parked():
    # one confirmed track, n_out 3: two parked rows; park at (-50, 70)
    c = call(*world(16, [(2, arc((3.0, 0.0), (0, 0), 0.3, 3))]), T=2, n_out=3, confirm=2, park_x=-50.0, park_y=70.0)
    z = dets_of(c)
    c["track"][0, 1] = (z[0, 0], z[0, 1], 0.0, 0.0)
    c["age"][0, 1] = 1
    return c


def nan_range():
    # the middle ray of five on one obstacle has a NaN range: two segments of two rays
    pts, rng = world(16, [(2, arc((3.0, 0.0), (0, 0), 0.3, 5))])
    rng[0, 4] = math.nan
    return call(pts, rng, gap=0.3, confirm=1)


CASES = {
    "seam_closed": lambda: seam(1), "seam_open": lambda: seam(0),
    "ring_closed": lambda: ring(1), "ring_open": lambda: ring(0),
    "gap_exact": lambda: gap_edge(False), "gap_beyond": lambda: gap_edge(True),
    "static_exact": lambda: static_edge(False), "static_below": lambda: static_edge(True),
    "drops_before_cap": lambda: many_segments(18, True, True), "seventeen": lambda: many_segments(17),
    "tie_jk": tie_jk, "gate_exact": lambda: gate_edge(False), "gate_beyond": lambda: gate_edge(True),
    "births": births, "full_slots": full_slots, "deletion": deletion, "clamp": clamp, "parked": parked,
    "nan_range": nan_range,
}
