"""The rules of localisation (include/rmpc.h: rmpc_grid_edge_distance_device, rmpc_lidar_project_device,
rmpc_scan_match_device) and of OdometryDrift.advance restated in numpy.  Rules only:
tests/test_localization_cpu.py checks them on hand-computed cases and in what they achieve,
tests/test_gpu_localization.py holds the device against them, bit for bit."""
import math

import numpy as np

from lidar_reference import sensor_origin


def fine_classes(grid, occ_threshold, sub):
    with np.errstate(invalid="ignore"):
        occ = np.asarray(grid, dtype=float) >= occ_threshold          # a NaN is not occupied
    return np.repeat(np.repeat(occ, sub, axis=0), sub, axis=1)


def edge_distance_ref(grid, occ_threshold, sub, cap):
    """rmpc_grid_edge_distance_device by brute force: every offset (dr, dc) with dr^2 + dc^2 < cap"""
    cls = fine_classes(grid, occ_threshold, sub)
    FH, FW = cls.shape
    d2 = np.full((FH, FW), cap, dtype=np.int32)
    w = math.isqrt(cap - 1) + 1                                        # ceil(sqrt(cap))
    for dr in range(-w, w + 1):
        for dc in range(-w, w + 1):
            d = dr * dr + dc * dc
            r0, r1, c0, c1 = max(0, -dr), min(FH, FH - dr), max(0, -dc), min(FW, FW - dc)
            if d == 0 or d >= cap or r0 >= r1 or c0 >= c1:
                continue
            other = cls[r0:r1, c0:c1] != cls[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
            view = d2[r0:r1, c0:c1]
            view[other] = np.minimum(view[other], d)
    return d2


def project_ref(pose, ranges, angle_min, angle_max, offset, height):
    """rmpc_lidar_project_device: points (B, R, 3), in scan_ref's expressions"""
    pose, t = np.asarray(pose, dtype=float), np.asarray(ranges, dtype=float)
    rays = t.shape[1]
    ox, oy = sensor_origin(pose[:, 0], pose[:, 1], pose[:, 2], offset)
    step = (angle_max - angle_min) / rays
    ang = (pose[:, 2:3] + angle_min) + np.arange(rays, dtype=float)[None, :] * step
    return np.stack([ox[:, None] + t * np.cos(ang), oy[:, None] + t * np.sin(ang), np.full_like(t, height)], axis=2)


def used_rays(points, ranges, max_range):
    with np.errstate(invalid="ignore"):
        return (np.isfinite(ranges) & np.isfinite(points[..., 0]) & np.isfinite(points[..., 1]) & (ranges > 0.0) &
                (ranges < max_range))


def fine_index(q, q0, cell, sub, n):
    """(index, inside): floor(((q - q0) / cell + 0.5) sub) compared as a double against [0, n)"""
    with np.errstate(invalid="ignore"):
        a = np.floor(((q - q0) / cell + 0.5) * float(sub))
        inside = (a >= 0.0) & (a < float(n))
    return np.where(inside, a, 0.0).astype(np.int64), inside


def match_ref(pose, points, ranges, max_range, d2, H, W, sub, cap, x0, y0, cell, nxy, step_xy, nth, step_th, rot,
              min_hits):
    """rmpc_scan_match_device: dict(pose_out (B, 3), best, score, score0, used (B,) int32).  The column of a ray's end
    depends on (jth, jx) alone and its row on (jth, jy): both are formed once, in the rule's own expressions."""
    pose, points, ranges = (np.asarray(a, dtype=float) for a in (pose, points, ranges))
    B, nx, nt = len(pose), 2 * nxy + 1, 2 * nth + 1
    ii = np.arange(nx) - nxy
    ith = np.arange(nt) - nth
    m = ith[:, None, None] ** 2 + ii[None, :, None] ** 2 + ii[None, None, :] ** 2
    kk = np.arange(nt * nx * nx, dtype=np.int64).reshape(nt, nx, nx)
    k0 = (nth * nx + nxy) * nx + nxy
    out = dict(pose_out=pose[:, :3].copy(), best=np.full(B, -1, np.int32), score=np.zeros(B, np.int32),
               score0=np.zeros(B, np.int32), used=np.zeros(B, np.int32))
    ok = used_rays(points, ranges, max_range)
    for b in range(B):
        x, y, th = pose[b, :3]
        n = int(ok[b].sum())
        out["used"][b] = n
        if n < min_hits:
            continue
        ux, uy = points[b, ok[b], 0] - x, points[b, ok[b], 1] - y
        c, s = rot[:, 0:1], rot[:, 1:2]
        with np.errstate(invalid="ignore"):
            qx = (c * ux - s * uy)[:, None, :] + (x + ii.astype(float) * step_xy)[None, :, None]      # (nt, nx, n)
            qy = (s * ux + c * uy)[:, None, :] + (y + ii.astype(float) * step_xy)[None, :, None]
        Ci, okc = fine_index(qx, x0, cell, sub, W * sub)
        Ri, okr = fine_index(qy, y0, cell, sub, H * sub)
        v = d2[Ri[:, :, None, :], Ci[:, None, :, :]]                                                  # (nt, jy, jx, n)
        v = np.where(okr[:, :, None, :] & okc[:, None, :, :], v, cap)
        sc = v.sum(axis=3, dtype=np.int64)
        k = int(np.argmin((sc << 25) | (m << 15) | kk))
        jth, jy, jx = k // (nx * nx), (k // nx) % nx, k % nx
        out["best"][b], out["score"][b], out["score0"][b] = k, sc[jth, jy, jx], sc.ravel()[k0]
        out["pose_out"][b] = (x + float(jx - nxy) * step_xy, y + float(jy - nxy) * step_xy, th + float(jth - nth) * step_th)
    return out


def match_literal(pose, points, ranges, max_range, d2, H, W, sub, cap, x0, y0, cell, nxy, step_xy, nth, step_th, rot,
                  min_hits):
    """The rule of one robot as written, a candidate and a ray at a time: (pose_out, best, score, score0, used)"""
    x, y, th = (float(v) for v in pose[:3])
    rays = [(float(p[0]) - x, float(p[1]) - y) for p, t in zip(points, ranges)
            if math.isfinite(t) and math.isfinite(p[0]) and math.isfinite(p[1]) and 0.0 < t < max_range]
    if len(rays) < min_hits:
        return (x, y, th), -1, 0, 0, len(rays)
    nx, best, score0 = 2 * nxy + 1, None, None
    for jth in range(2 * nth + 1):
        c, s = float(rot[jth, 0]), float(rot[jth, 1])
        for jy in range(nx):
            for jx in range(nx):
                ith, iy, ix = jth - nth, jy - nxy, jx - nxy
                sc = 0
                for ux, uy in rays:
                    qx = (c * ux - s * uy) + (x + ix * step_xy)
                    qy = (s * ux + c * uy) + (y + iy * step_xy)
                    a, r = ((qx - x0) / cell + 0.5) * sub, ((qy - y0) / cell + 0.5) * sub
                    inside = 0.0 <= math.floor(a) < W * sub and 0.0 <= math.floor(r) < H * sub if \
                        math.isfinite(a) and math.isfinite(r) else False
                    sc += int(d2[math.floor(r), math.floor(a)]) if inside else cap
                key = (sc, ix * ix + iy * iy + ith * ith, (jth * nx + jy) * nx + jx)
                if ix == 0 and iy == 0 and ith == 0:
                    score0 = sc
                if best is None or key < best[0]:
                    best = (key, (x + ix * step_xy, y + iy * step_xy, th + ith * step_th))
    return best[1], best[0][2], best[0][0], score0, len(rays)


def advance_ref(est, x_prev, x_new, noise, sigma_ds=0.05, sigma_dth=0.01, bias_dth=0.002):
    """OdometryDrift.advance on numpy arrays, noise (B, 2) the step's rows of the table; returns the new estimate"""
    th = x_prev[:, 2]
    ds = (x_new[:, 0] - x_prev[:, 0]) * np.cos(th) + (x_new[:, 1] - x_prev[:, 1]) * np.sin(th)
    ds = ds * (1.0 + sigma_ds * noise[:, 0])
    dth = (x_new[:, 2] - th) + sigma_dth * noise[:, 1] + bias_dth
    return np.stack([est[:, 0] + ds * np.cos(est[:, 2]), est[:, 1] + ds * np.sin(est[:, 2]), est[:, 2] + dth], axis=1)


def wrap(a):
    return (a + math.pi) % (2.0 * math.pi) - math.pi
