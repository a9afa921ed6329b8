"""The fleet scan's rule (include/rmpc.h, rmpc_lidar_bodies) restated in numpy on top of
lidar_reference.scan_ref: the static world first, then one plain loop over the bodies, no cull.  Rules only:
tests/test_lidar_fleet_cpu.py checks them on hand-computed cases, tests/test_gpu_lidar_fleet.py holds the device against
them."""
import numpy as np

from lidar_reference import scan_ref, sensor_origin

EPS = 2.3e-16


def fleet_scan_ref(pose, rays, angle_min, angle_max, max_range, offset=(0.4, 0.0), height=0.02, boxes=None,
                   circles=None, centres=None, radius=None, self0=0, near_tol=1e-9):
    """pose (B, >= 3), centres (P, >= 2), radius (P,) -> dict(points (B, R, 3), ranges, static_ranges (B, R), owner
    (B, R) int32, near, sensitive, ambiguous, body_hits (B, R) bool).  near: scan_ref's mark extended to the bodies (a
    candidate within near_tol of tangency in front of the sensor); sensitive: the winning body's hit moves by more
    than 1e-13 m with a last-bit change of the direction (|u| EPS |bb| / sqrt(disc)); ambiguous: a second candidate,
    static or body, within 1e-9 of t; body_hits: some body passed the circle rule, whether it won or not."""
    pose = np.asarray(pose, dtype=float)
    B = pose.shape[0]
    centres = np.zeros((0, 2)) if centres is None or len(centres) == 0 else np.asarray(centres, dtype=float)
    radius = np.zeros(0) if radius is None else np.asarray(radius, dtype=float)
    _, ts, near = scan_ref(pose, rays, angle_min, angle_max, max_range, offset, height, boxes, circles, near_tol)
    near = near.copy()
    ox, oy = sensor_origin(pose[:, 0], pose[:, 1], pose[:, 2], offset)
    ox, oy = ox[:, None], oy[:, None]
    step = (angle_max - angle_min) / rays
    ang = (pose[:, 2:3] + angle_min) + np.arange(rays, dtype=float)[None, :] * step
    dx, dy = np.cos(ang), np.sin(ang)
    t = ts.copy()
    owner = np.full((B, rays), -1, dtype=np.int64)
    sens = np.zeros((B, rays), dtype=bool)          # of the current winner
    second = np.full((B, rays), np.inf)             # the least candidate distance that did not win
    body_hits = np.zeros((B, rays), dtype=bool)     # some body passed the circle rule, whether it won or not
    robot = np.arange(B)[:, None]
    with np.errstate(invalid="ignore"):
        for j in range(len(radius)):
            cx, cy, r = centres[j, 0], centres[j, 1], radius[j]
            if not r > 0.0:
                continue
            ux, uy = ox - cx, oy - cy
            bb = dx * ux + dy * uy
            cc = (ux * ux + uy * uy) - r * r
            disc = bb * bb - cc
            ok = (cc > 0.0) & (disc >= 0.0) & (robot != j - self0)
            tc = -bb - np.sqrt(np.where(ok, disc, 0.0))
            hit = ok & (tc > 0.0)
            body_hits |= hit
            win = hit & ((tc < t) | ((tc == t) & (owner >= 0) & (j < owner)))
            second = np.where(win, np.minimum(second, t), np.where(hit, np.minimum(second, tc), second))
            s = np.hypot(ux, uy) * EPS * np.abs(bb) > 1e-13 * np.sqrt(np.maximum(disc, 1e-300))
            sens = np.where(win, s, sens)
            t = np.where(win, tc, t)
            owner = np.where(win, j, owner)
            near |= (robot != j - self0) & (np.abs(np.abs(dx * uy - dy * ux) - r) <= near_tol) & (-bb > -near_tol)
    # a body that won pushed the static hit into `second`; where the static world won, the bodies' hits are in it
    owner = np.where(owner >= 0, owner, np.where(ts < max_range, -2, -1)).astype(np.int32)
    ambiguous = np.abs(second - t) <= 1e-9
    points = np.stack([ox + t * dx, oy + t * dy, np.full_like(t, height)], axis=2)
    return dict(points=points, ranges=t, static_ranges=ts, owner=owner, near=near, sensitive=sens & (owner >= 0),
                ambiguous=ambiguous, body_hits=body_hits)
