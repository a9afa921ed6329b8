"""The rules of the map built from lidar scans (include/rmpc.h, rmpc_grid_mark_device and rmpc_grid_occupancy_device;
DESIGN.md 14) restated in numpy.  Rules only: tests/test_mapping_cpu.py checks them on hand-computed cases and against
the true map of seeded stores, tests/test_gpu_mapping.py holds the device against them, integer for integer."""
import math

import numpy as np

INF = math.inf


def ray_cells(o, e, t, x0, y0, cell, max_range, hit_depth):
    """One ray in plain Python floats: None when the ray is skipped, else (cells, hit) with cells the n + 1 visited
    (row, col) in order, cells outside the map included."""
    ox, oy, ex, ey, t = float(o[0]), float(o[1]), float(e[0]), float(e[1]), float(t)
    if not (all(math.isfinite(v) for v in (ox, oy, ex, ey, t)) and 0.0 < t <= max_range):
        return None
    hit = t < max_range
    if hit:
        s = hit_depth / t
        ex = ex + s * (ex - ox)
        ey = ey + s * (ey - oy)
    ua, va = (ox - x0) / cell + 0.5, (oy - y0) / cell + 0.5
    ub, vb = (ex - x0) / cell + 0.5, (ey - y0) / cell + 0.5
    if not all(math.isfinite(v) for v in (ua, va, ub, vb)):
        return None                      # (n is then not a number: the test n <= limit fails)
    c, r, c1, r1 = math.floor(ua), math.floor(va), math.floor(ub), math.floor(vb)
    n = abs(c1 - c) + abs(r1 - r)
    if not n <= 2 * math.ceil((max_range + hit_depth) / cell) + 4:
        return None
    du, dv = ub - ua, vb - va
    sc, sr = (1 if du > 0 else -1), (1 if dv > 0 else -1)
    tx = ((c + (1 if du > 0 else 0)) - ua) / du if du != 0 else INF
    ty = ((r + (1 if dv > 0 else 0)) - va) / dv if dv != 0 else INF
    cells = [(r, c)]
    for _ in range(n):
        if (tx <= ty and c != c1) or r == r1:
            c += sc
            tx = ((c + (1 if du > 0 else 0)) - ua) / du
        else:
            r += sr
            ty = ((r + (1 if dv > 0 else 0)) - va) / dv
        cells.append((r, c))
    assert cells[-1] == (r1, c1) and len(set(cells)) == n + 1
    return cells, hit


def mark_ref(origins, points, ranges, H, W, x0, y0, cell, max_range, hit_depth, hits=None, misses=None):
    """rmpc_grid_mark_device for all rays at once: origins (B, 3) or (B, 1, 3), points (B, R, 3), ranges (B, R) ->
    (hits (H, W) int64, misses (H, W) int64, skipped).  hits and misses, when given, are added to in place.  The same
    expressions as ``ray_cells`` in float64; cell coordinates stay floats (exact integers) so that a ray far outside
    the map walks like any other."""
    o = np.asarray(origins, dtype=float).reshape(-1, 3)
    B = o.shape[0]
    p = np.asarray(points, dtype=float).reshape(B, -1, 3)
    R = p.shape[1]
    t = np.asarray(ranges, dtype=float).reshape(B * R)
    hits = np.zeros((H, W), dtype=np.int64) if hits is None else hits
    misses = np.zeros((H, W), dtype=np.int64) if misses is None else misses
    ox, oy = np.repeat(o[:, 0], R), np.repeat(o[:, 1], R)
    ex, ey = p[:, :, 0].reshape(-1), p[:, :, 1].reshape(-1)
    with np.errstate(all="ignore"):
        ok = np.isfinite(ox) & np.isfinite(oy) & np.isfinite(ex) & np.isfinite(ey) & np.isfinite(t) & (t > 0.0) & (t <= max_range)
        hit = ok & (t < max_range)
        s = hit_depth / t
        ex = np.where(hit, ex + s * (ex - ox), ex)
        ey = np.where(hit, ey + s * (ey - oy), ey)
        ua, va = (ox - x0) / cell + 0.5, (oy - y0) / cell + 0.5
        ub, vb = (ex - x0) / cell + 0.5, (ey - y0) / cell + 0.5
        c, r, c1, r1 = np.floor(ua), np.floor(va), np.floor(ub), np.floor(vb)
        n = np.abs(c1 - c) + np.abs(r1 - r)
        ok &= n <= 2 * math.ceil((max_range + hit_depth) / cell) + 4       # False for a NaN
        skipped = int((~ok).sum())
        ua, va, ub, vb, c, r, c1, r1, n, hit = (a[ok] for a in (ua, va, ub, vb, c, r, c1, r1, n, hit))
        du, dv = ub - ua, vb - va
        pc, pr = (du > 0).astype(float), (dv > 0).astype(float)
        sc, sr = np.where(du > 0, 1.0, -1.0), np.where(dv > 0, 1.0, -1.0)
        tx = np.where(du != 0, ((c + pc) - ua) / du, INF)
        ty = np.where(dv != 0, ((r + pr) - va) / dv, INF)
        for k in range(int(n.max()) + 1 if len(n) else 0):
            inside = (k <= n) & (r >= 0) & (r < H) & (c >= 0) & (c < W)
            end = inside & hit & (k == n)
            for sel, out in ((end, hits), (inside & ~end, misses)):
                idx = r[sel].astype(np.int64) * W + c[sel].astype(np.int64)
                out += np.bincount(idx, minlength=H * W).reshape(H, W)
            col = (k < n) & (((tx <= ty) & (c != c1)) | (r == r1))
            row = (k < n) & ~col
            c = np.where(col, c + sc, c)
            tx = np.where(col, ((c + pc) - ua) / du, tx)
            r = np.where(row, r + sr, r)
            ty = np.where(row, ((r + pr) - va) / dv, ty)
    return hits, misses, skipped


def occupancy_ref(hits, misses, w_hit, w_miss, forget, free_value, occ_value, unknown_value):
    """rmpc_grid_occupancy_device: (grid (H, W) float64, hits and misses after the ageing shift)"""
    h, m = np.asarray(hits).astype(np.int64), np.asarray(misses).astype(np.int64)
    grid = np.where(h + m == 0, unknown_value, np.where(h * w_hit > m * w_miss, occ_value, free_value))
    return grid, h >> forget, m >> forget
