"""The moving-obstacle tracker's rules (include/rmpc.h, rmpc_tracks) restated in numpy and plain Python,
written from the header's text: every floating-point expression in the header's order, one operation at a time, on IEEE
doubles.  tests/test_tracking_cpu.py pins it on hand-worked cases, tests/test_gpu_tracking.py holds the device to it bit
for bit."""
import math

import numpy as np

MAX_RAYS, MAX_TRACKS, MAX_DET = 2048, 16, 16
I32_MAX = 2 ** 31 - 1

DEFAULTS = dict(closed=1, min_rays=2, range=10.0, margin=0.05, gap=0.3, radius=0.3, max_extent=0.0, gate=1.0, dt=0.1,
                alpha=0.4, beta=0.1, v_max=0.0, park_x=100.0, park_y=100.0, confirm=3, max_miss=5)


def params(**kw):
    """The scalars of one call; unknown names are refused"""
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else math.nan


def _div(a, b):
    """a / b as IEEE does it (Python raises on a zero divisor)"""
    return float(np.float64(a) / np.float64(b))


def moving_rays(ranges, static_ranges, p):
    """(R,) bool, rule 1"""
    with np.errstate(invalid="ignore"):
        if static_ranges is None:
            return ranges < p["range"]
        return ranges < static_ranges - p["margin"]


def segments(pts, moving, p):
    """rule 2: (all segments as (start, n) in start order, the detections' segments)"""
    R = len(moving)
    closed = bool(p["closed"])
    gap2 = p["gap"] * p["gap"]
    start = np.zeros(R, dtype=bool)
    for i in range(R):
        if not moving[i]:
            continue
        pred = i - 1 if i > 0 else (R - 1 if closed else -1)
        link = False
        if pred >= 0 and moving[pred]:
            dx, dy = pts[i][0] - pts[pred][0], pts[i][1] - pts[pred][1]
            link = (dx * dx + dy * dy) <= gap2
        start[i] = not link
    if closed and moving.all() and not start.any():
        start[0] = True
    segs = []
    for s in np.flatnonzero(start):
        n = 1
        while n < R:
            j = s + n
            if j >= R:
                if not closed:
                    break
                j -= R
            if start[j] or not moving[j]:
                break
            n += 1
        segs.append((int(s), n))
    kept = []
    me2 = p["max_extent"] * p["max_extent"]
    for s, n in segs:
        if n < p["min_rays"]:
            continue
        if p["max_extent"] > 0.0:
            a, b = pts[s], pts[(s + n - 1) % R]
            dx, dy = b[0] - a[0], b[1] - a[1]
            if (dx * dx + dy * dy) > me2:
                continue
        kept.append((s, n))
    return segs, kept[:MAX_DET]


def fit_circle(pts, s, n, o, radius):
    """rule 3: the centre of the circle of the known radius through the n points from ray s on"""
    R = len(pts)
    P = [(float(pts[(s + t) % R][0]), float(pts[(s + t) % R][1])) for t in range(n)]
    sx = sy = 0.0
    for x, y in P:
        sx = sx + x
        sy = sy + y
    mx, my = sx / float(n), sy / float(n)
    wx, wy = mx - o[0], my - o[1]
    nrm = _sqrt(wx * wx + wy * wy)
    cx = mx + radius * _div(wx, nrm)
    cy = my + radius * _div(wy, nrm)
    for _ in range(4):
        a11 = a12 = a22 = gx = gy = 0.0
        for x, y in P:
            qx, qy = x - cx, y - cy
            r = _sqrt(qx * qx + qy * qy)
            ux, uy = _div(qx, r), _div(qy, r)
            e = r - radius
            a11 = a11 + ux * ux
            a12 = a12 + ux * uy
            a22 = a22 + uy * uy
            gx = gx + ux * e
            gy = gy + uy * e
        a11 = a11 + 1e-3
        a22 = a22 + 1e-3
        D = a11 * a22 - a12 * a12
        cx = cx + _div(a22 * gx - a12 * gy, D)
        cy = cy + _div(a11 * gy - a12 * gx, D)
    return cx, cy


def detect(pts, ranges, static_ranges, o, p):
    """rules 1 to 3 of one robot: (det (n, 2), segments found, the kept segments)"""
    mv = moving_rays(ranges, static_ranges, p)
    segs, kept = segments(pts, mv, p)
    det = np.zeros((len(kept), 2))
    for k, (s, n) in enumerate(kept):
        det[k] = fit_circle(pts, s, n, o, p["radius"])
    return det, len(segs), kept


def associate(pred, live, det, gate):
    """rule 4's greedy pairing: (match of slot j or -1, match of detection k or -1)"""
    T, K = len(live), len(det)
    g2 = gate * gate
    cand = []
    for j in range(T):
        if not live[j]:
            continue
        for k in range(K):
            dx, dy = pred[j][0] - det[k][0], pred[j][1] - det[k][1]
            s = dx * dx + dy * dy
            if s <= g2:
                cand.append((s, j, k))
    cand.sort()
    mj, mk = [-1] * T, [-1] * K
    for s, j, k in cand:
        if mj[j] < 0 and mk[k] < 0:
            mj[j], mk[k] = k, j
    return mj, mk


def track_update(track, age, miss, det, o, p, n_out):
    """rules 4 and 5 of one robot, in place on track (T, 4), age, miss (T,); returns (obst_dyn (n_out, 9), live,
    confirmed)"""
    T = len(age)
    dt, alpha, beta, vmax = p["dt"], p["alpha"], p["beta"], p["v_max"]
    live = [int(age[j]) > 0 for j in range(T)]
    pred = [(float(track[j][0]) + float(track[j][2]) * dt, float(track[j][1]) + float(track[j][3]) * dt) for j in range(T)]
    mj, mk = associate(pred, live, det, p["gate"])
    for j in range(T):
        if not live[j]:
            continue
        if mj[j] >= 0:
            z = det[mj[j]]
            for c in range(2):
                res = float(z[c]) - pred[j][c]
                v = float(track[j][2 + c]) + _div(beta * res, dt)
                if vmax > 0.0:
                    if v > vmax:
                        v = vmax
                    if v < -vmax:
                        v = -vmax
                track[j][c] = pred[j][c] + alpha * res
                track[j][2 + c] = v
            age[j] = min(int(age[j]) + 1, I32_MAX)
            miss[j] = 0
        else:
            track[j][0], track[j][1] = pred[j]
            miss[j] = min(int(miss[j]) + 1, I32_MAX)
            if int(miss[j]) > p["max_miss"]:
                age[j] = 0
    for k in range(len(det)):
        if mk[k] >= 0:
            continue
        free = [j for j in range(T) if int(age[j]) == 0]
        if not free:
            break
        j = free[0]
        track[j] = (det[k][0], det[k][1], 0.0, 0.0)
        age[j], miss[j] = 1, 0
    conf = []
    for j in range(T):
        if int(age[j]) >= p["confirm"]:
            dx, dy = float(track[j][0]) - o[0], float(track[j][1]) - o[1]
            s = dx * dx + dy * dy
            conf.append((s if s == s else math.inf, j))
    conf.sort()
    out = np.zeros((n_out, 9))
    out[:, 0], out[:, 1] = p["park_x"], p["park_y"]
    for row, (_, j) in enumerate(conf[:n_out]):
        out[row] = (track[j][0], track[j][1], 0.0, track[j][2], track[j][3], 0.0, 0.0, 0.0, 0.0)
    return out, sum(int(a) > 0 for a in age), len(conf)


def tracks_ref(points, ranges, static_ranges, origin, p, track, age, miss, n_out):
    """One call of rmpc_lidar_tracks_device for B robots: points (B, R, 3), ranges (B, R), static_ranges (B, R) or None,
    origin (B, 3); track (B, T, 4), age, miss (B, T) int32 are updated in place.  Returns obst_dyn (B, n_out, 9), det
    (B, MAX_DET, 2) and counts (B, 4) int32."""
    B = points.shape[0]
    obst = np.zeros((B, n_out, 9))
    det = np.zeros((B, MAX_DET, 2))
    counts = np.zeros((B, 4), dtype=np.int32)
    with np.errstate(all="ignore"):
        for b in range(B):
            o = (float(origin[b, 0]), float(origin[b, 1]))
            d, nseg, kept = detect(points[b, :, :2], ranges[b], None if static_ranges is None else static_ranges[b], o, p)
            det[b, :len(d)] = d
            obst[b], nlive, nconf = track_update(track[b], age[b], miss[b], d, o, p, n_out)
            counts[b] = (nseg, len(kept), nlive, nconf)
    return obst, det, counts
