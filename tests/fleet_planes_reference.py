"""Fleet separation's rules (include/rmpc.h, rmpc_fleet_points_device / rmpc_fleet_planes_device)
restated in numpy.  Rules only: tests/test_fleet_planes_cpu.py checks them on hand-computed cases and by sampling,
tests/test_gpu_fleet_planes.py holds the device against them."""
import math

import numpy as np


def fleet_points_ref(pose, N, z_prev=None, exitflag=None, heading=1, offset=(0.4, 0.0), height=0.0):
    """(B, N, 3) predicted collision points: stage min(k + 1, N - 1) of z_prev, the pose when there is no plan or
    exitflag < 0; heading 1 = the point `offset` ahead in the body frame, 0 = (q0, q1)."""
    pose = np.asarray(pose, dtype=float)
    B = pose.shape[0]
    out = np.zeros((B, N, 3))
    kk = np.minimum(np.arange(N) + 1, N - 1)
    for b in range(B):
        plan = z_prev is not None and (exitflag is None or exitflag[b] >= 0)
        q = np.asarray(z_prev[b, kk, :3], dtype=float) if plan else np.repeat(pose[b:b + 1, :3], N, axis=0)
        if heading:
            c, s = np.cos(q[:, 2]), np.sin(q[:, 2])
            out[b, :, 0] = q[:, 0] + offset[0] * c - offset[1] * s
            out[b, :, 1] = q[:, 1] + offset[0] * s + offset[1] * c
        else:
            out[b, :, 0], out[b, :, 1] = q[:, 0], q[:, 1]
        out[b, :, 2] = height
    return out


def dummy_plane(q):
    """k_fsd's HalfPlane(seed + (20, 20, 0), seed)"""
    p = np.array([q[0] + 20.0, q[1] + 20.0, q[2] + 0.0])
    n = np.asarray(q, dtype=float) - p
    return np.array([n[0], n[1], n[2], -((n[0] * p[0] + n[1] * p[1]) + n[2] * p[2])])


def pair_plane(q_lo, q_hi, r_lo, r_hi):
    """(n, c) of the pair as robot lo holds it"""
    u = np.asarray(q_lo, dtype=float) - np.asarray(q_hi, dtype=float)
    d = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    n = np.array([1.0, 0.0, 0.0]) if d == 0.0 else u / d
    g = d - r_lo - r_hi
    m = q_hi + (r_hi + 0.5 * g) * n
    return np.array([n[0], n[1], n[2], -((n[0] * m[0] + n[1] * m[1]) + n[2] * m[2])])


def neighbours_ref(points, K, max_range):
    """(B, N, K) int: the selected j per slot, -1 where there is no candidate"""
    B, N = points.shape[:2]
    r2 = max_range * max_range
    sel = np.full((B, N, K), -1, dtype=np.int64)
    for k in range(N):
        q = points[:, k]
        for b in range(B):
            u = q - q[b]
            s = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
            s[b] = math.inf
            cand = np.flatnonzero(s < r2)
            cand = cand[np.argsort(s[cand], kind="stable")][:K]
            sel[b, k, :len(cand)] = cand
    return sel


def fleet_planes_ref(points, radius, K, max_range, nobst=None, slot0=0, planes=None):
    """(B, N, nobst, 4): slots slot0 .. slot0 + K - 1 written, the others taken from `planes` (zeros if None)"""
    points = np.asarray(points, dtype=float)
    B, N = points.shape[:2]
    nobst = slot0 + K if nobst is None else nobst
    out = np.zeros((B, N, nobst, 4)) if planes is None else np.array(planes, dtype=float, copy=True)
    sel = neighbours_ref(points, K, max_range)
    for b in range(B):
        for k in range(N):
            for s in range(K):
                j = sel[b, k, s]
                if j < 0:
                    out[b, k, slot0 + s] = dummy_plane(points[b, k])
                else:
                    lo, hi = min(b, j), max(b, j)
                    p = pair_plane(points[lo, k], points[hi, k], radius[lo], radius[hi])
                    out[b, k, slot0 + s] = p if b == lo else -p
    return out
