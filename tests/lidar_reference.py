"""The lidar's rules (include/rmpc.h, rmpc_lidar) restated in numpy: the scan of boxes and circles and the
per-stage seed points.  Rules only: tests/test_lidar_cpu.py checks them on hand-computed cases, tests/test_gpu_lidar.py
holds the device against them."""
import math

import numpy as np

INF = math.inf


def sensor_origin(x, y, th, offset):
    c, s = np.cos(th), np.sin(th)
    return x + offset[0] * c - offset[1] * s, y + offset[0] * s + offset[1] * c


def scan_ref(pose, rays, angle_min, angle_max, max_range, offset=(0.4, 0.0), height=0.02, boxes=None, circles=None,
             near_tol=1e-9):
    """pose (B, >= 3) -> (points (B, R, 3), ranges (B, R), near (B, R)).  near marks the rays whose outcome a last-bit
    difference of sin / cos may change: a box corner within near_tol of the ray, or a circle within near_tol of
    tangency (in front of the sensor)."""
    pose = np.asarray(pose, dtype=float)
    B = pose.shape[0]
    ox, oy = sensor_origin(pose[:, 0], pose[:, 1], pose[:, 2], offset)
    ox, oy = ox[:, None], oy[:, None]
    step = (angle_max - angle_min) / rays
    ang = (pose[:, 2:3] + angle_min) + np.arange(rays, dtype=float)[None, :] * step
    dx, dy = np.cos(ang), np.sin(ang)
    zx, zy = dx == 0.0, dy == 0.0
    ix = np.where(zx, 0.0, 1.0 / np.where(zx, 1.0, dx))
    iy = np.where(zy, 0.0, 1.0 / np.where(zy, 1.0, dy))
    t = np.full((B, rays), float(max_range))
    near = np.zeros((B, rays), dtype=bool)

    def near_point(px, py):
        ux, uy = px - ox, py - oy
        along = dx * ux + dy * uy
        return (np.abs(dx * uy - dy * ux) <= near_tol) & (along > -near_tol) & (along <= max_range + near_tol)

    for cx, cy, lx, ly in (np.zeros((0, 4)) if boxes is None else np.asarray(boxes, dtype=float)):
        hx, hy = 0.5 * lx, 0.5 * ly
        x0, x1, y0, y1 = cx - hx, cx + hx, cy - hy, cy + hy
        ax, bx = (x0 - ox) * ix, (x1 - ox) * ix
        ay, by = (y0 - oy) * iy, (y1 - oy) * iy
        nx, fx, ny, fy = np.minimum(ax, bx), np.maximum(ax, bx), np.minimum(ay, by), np.maximum(ay, by)
        nx = np.where(zx, np.where((ox >= x0) & (ox <= x1), -INF, INF), nx)
        fx = np.where(zx, INF, fx)
        ny = np.where(zy, np.where((oy >= y0) & (oy <= y1), -INF, INF), ny)
        fy = np.where(zy, INF, fy)
        te, tx = np.maximum(nx, ny), np.minimum(fx, fy)
        t = np.where((te > 0.0) & (te <= tx) & (te < t), te, t)
        for px, py in ((x0, y0), (x0, y1), (x1, y0), (x1, y1)):
            near |= near_point(px, py)
    for cx, cy, r in (np.zeros((0, 3)) if circles is None else np.asarray(circles, dtype=float)):
        ux, uy = ox - cx, oy - cy
        bb = dx * ux + dy * uy
        cc = (ux * ux + uy * uy) - r * r
        disc = bb * bb - cc
        ok = (cc > 0.0) & (disc >= 0.0)
        tc = -bb - np.sqrt(np.where(ok, disc, 0.0))
        t = np.where(ok & (tc > 0.0) & (tc < t), tc, t)
        near |= (np.abs(np.abs(dx * uy - dy * ux) - r) <= near_tol) & (-bb > -near_tol)
    points = np.stack([ox + t * dx, oy + t * dy, np.full_like(t, height)], axis=2)
    return points, t, near


def plan_points_ref(pose, N, z_prev=None, exitflag=None, offset=(0.4, 0.0), height=0.02):
    """(B, N, 3) seeds: the sensor origin of z_prev [b][k][0 .. 2], of the pose when there is no plan or exitflag < 0."""
    pose = np.asarray(pose, dtype=float)
    B = pose.shape[0]
    out = np.zeros((B, N, 3))
    for b in range(B):
        plan = z_prev is not None and (exitflag is None or exitflag[b] >= 0)
        q = np.asarray(z_prev[b, :, :3], dtype=float) if plan else np.repeat(pose[b:b + 1, :3], N, axis=0)
        ox, oy = sensor_origin(q[:, 0], q[:, 1], q[:, 2], offset)
        out[b] = np.stack([ox, oy, np.full(N, height)], axis=1)
    return out
