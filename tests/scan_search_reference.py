"""The rules of wide-window localisation (include/rmpc.h: rmpc_grid_min_pyramid_device, rmpc_scan_search_device;
DESIGN.md 21) restated in numpy.  Rules only: tests/test_scan_search_cpu.py checks that the bound is one and that a
search on it returns the exhaustive rule's result, tests/test_gpu_scan_search.py holds the device against them, bit
for bit.  The geometry of a launch is the keyword set of localization_reference.match_ref."""
import heapq

import numpy as np

from localization_reference import used_rays


# ---- the pyramid ---------------------------------------------------------------------------------------------------------
def min_pyramid_ref(d2, levels):
    """rmpc_grid_min_pyramid_device: (levels, FH, FW) int32, each level from the one below by four reads"""
    d2 = np.asarray(d2, dtype=np.int32)
    FH, FW = d2.shape
    pyr = np.empty((levels, FH, FW), dtype=np.int32)
    pyr[0] = d2
    for l in range(1, levels):
        h, src, v = 1 << (l - 1), pyr[l - 1], pyr[l - 1].copy()
        if h < FW:
            v[:, :FW - h] = np.minimum(v[:, :FW - h], src[:, h:])
        if h < FH:
            v[:FH - h, :] = np.minimum(v[:FH - h, :], src[h:, :])
        if h < FW and h < FH:
            v[:FH - h, :FW - h] = np.minimum(v[:FH - h, :FW - h], src[h:, h:])
        pyr[l] = v
    return pyr


def min_pyramid_literal(d2, levels):
    """the definition: per level l and cell (R, C) the least d2 over [R, R + 2^l) x [C, C + 2^l) inside the map, one
    offset of the window at a time"""
    d2 = np.asarray(d2, dtype=np.int32)
    FH, FW = d2.shape
    pyr = np.empty((levels, FH, FW), dtype=np.int32)
    for l in range(levels):
        v = d2.copy()
        for dr in range(min(1 << l, FH)):
            for dc in range(min(1 << l, FW)):
                v[:FH - dr, :FW - dc] = np.minimum(v[:FH - dr, :FW - dc], d2[dr:, dc:])
        pyr[l] = v
    return pyr


# ---- a robot's rays ------------------------------------------------------------------------------------------------------
def _fine(q, q0, cell, sub):
    """rule 4's fine coordinate as a double"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor(((q - q0) / cell + 0.5) * float(sub))


def _rays_of(pose_b, points_b, ranges_b, max_range):
    ok = used_rays(points_b, ranges_b, max_range)
    return points_b[ok, 0] - pose_b[0], points_b[ok, 1] - pose_b[1]


def _m_and_k(nxy, nth):
    nx = 2 * nxy + 1
    ii = (np.arange(nx) - nxy) ** 2
    return ii[:, None] + ii[None, :], nx


# ---- the exhaustive rule -------------------------------------------------------------------------------------------------
def rotation_scores(ux, uy, x, y, c, s, d2, H, W, sub, cap, x0, y0, cell, nxy, step_xy):
    """rules 3 and 4 for one rotation (c, s): the scores (jy, jx) int64 of its (2 nxy + 1)^2 candidates"""
    ii = (np.arange(2 * nxy + 1) - nxy).astype(float)
    with np.errstate(invalid="ignore", over="ignore"):
        qx = (c * ux - s * uy)[None, :] + (x + ii * step_xy)[:, None]                                  # (nx, n)
        qy = (s * ux + c * uy)[None, :] + (y + ii * step_xy)[:, None]
        Cf, Rf = _fine(qx, x0, cell, sub), _fine(qy, y0, cell, sub)
        okc, okr = (Cf >= 0.0) & (Cf < float(W * sub)), (Rf >= 0.0) & (Rf < float(H * sub))
    Ci, Ri = np.where(okc, Cf, 0.0).astype(np.int64), np.where(okr, Rf, 0.0).astype(np.int64)
    v = np.where(okr[:, None, :] & okc[None, :, :], d2[Ri[:, None, :], Ci[None, :, :]], cap)          # (jy, jx, n)
    return v.sum(axis=2, dtype=np.int64)


def scores_ref(pose_b, points_b, ranges_b, max_range, d2, H, W, sub, cap, x0, y0, cell, nxy, step_xy, nth, step_th, rot,
               min_hits):
    """every candidate's score of one robot, (2 nth + 1, jy, jx) int64, and m of the same shape"""
    pose_b, points_b, ranges_b = (np.asarray(a, dtype=float) for a in (pose_b, points_b, ranges_b))
    ux, uy = _rays_of(pose_b, points_b, ranges_b, max_range)
    sc = np.stack([rotation_scores(ux, uy, pose_b[0], pose_b[1], rot[j, 0], rot[j, 1], d2, H, W, sub, cap, x0, y0, cell, nxy,
                                   step_xy) for j in range(2 * nth + 1)])
    return sc, _m_and_k(nxy, nth)[0][None] + ((np.arange(2 * nth + 1) - nth) ** 2)[:, None, None]


def match_wide_ref(pose, points, ranges, max_range, d2, H, W, sub, cap, x0, y0, cell, nxy, step_xy, nth, step_th, rot,
                   min_hits, active=None):
    """Rules 1 to 5 of rmpc_scan_match over a lattice of any width, the order (score, m, k) as a tuple: dict(pose_out
    (B, 3), best, score, score0, used (B,) int32).  One rotation at a time."""
    pose, points, ranges = (np.asarray(a, dtype=float) for a in (pose, points, ranges))
    B = len(pose)
    mxy, nx = _m_and_k(nxy, nth)
    kxy = np.arange(nx * nx, dtype=np.int64).reshape(nx, nx)
    out = dict(pose_out=pose[:, :3].copy(), best=np.full(B, -1, np.int32), score=np.zeros(B, np.int32),
               score0=np.zeros(B, np.int32), used=np.zeros(B, np.int32))
    for b in range(B):
        x, y, th = pose[b, :3]
        ux, uy = _rays_of(pose[b], points[b], ranges[b], max_range)
        out["used"][b] = len(ux)
        if len(ux) < min_hits or (active is not None and active[b] == 0):
            continue
        best = None
        for jth in range(2 * nth + 1):
            sc = rotation_scores(ux, uy, x, y, rot[jth, 0], rot[jth, 1], d2, H, W, sub, cap, x0, y0, cell, nxy, step_xy)
            if jth == nth:
                out["score0"][b] = sc[nxy, nxy]
            m = mxy + (jth - nth) ** 2
            least = sc == sc.min()
            least &= m == m[least].min()
            key = (int(sc.min()), int(m[least].min()), jth * nx * nx + int(kxy[least].min()))
            if best is None or key < best:
                best = key
        k = best[2]
        jth, jy, jx = k // (nx * nx), (k // nx) % nx, k % nx
        out["best"][b], out["score"][b] = k, best[0]
        out["pose_out"][b] = (x + float(jx - nxy) * step_xy, y + float(jy - nxy) * step_xy, th + float(jth - nth) * step_th)
    return out


# ---- the bound -----------------------------------------------------------------------------------------------------------
class Robot:
    """one robot's used rays and the launch's geometry, for node_bound_ref"""

    def __init__(self, pose_b, points_b, ranges_b, pyr, max_range, d2, H, W, sub, cap, x0, y0, cell, nxy, step_xy, nth,
                 step_th, rot, min_hits):
        self.x, self.y, self.th = (float(v) for v in pose_b[:3])
        self.ux, self.uy = _rays_of(np.asarray(pose_b, float), np.asarray(points_b, float), np.asarray(ranges_b, float),
                                    max_range)
        self.pyr, self.levels = pyr, len(pyr)
        self.FH, self.FW, self.sub, self.cap = H * sub, W * sub, sub, cap
        self.x0, self.y0, self.cell = x0, y0, cell
        self.nxy, self.nth, self.nx, self.step_xy, self.rot = nxy, nth, 2 * nxy + 1, step_xy, np.asarray(rot)


def node_bound_ref(r, jth, a, a1, b, b1):
    """The bounds of the nodes (jth, [a, a1], [b, b1]) (int arrays of one shape (N,)) of Robot r, int64 (N,): the formula
    of include/rmpc.h.  A node with a == a1 and b == b1 is a leaf and gets rule 4's exact score."""
    jth, a, a1, b, b1 = (np.asarray(v, dtype=np.int64) for v in (jth, a, a1, b, b1))
    c, s = r.rot[jth, 0][:, None], r.rot[jth, 1][:, None]
    fw, fh = float(r.FW), float(r.FH)
    with np.errstate(invalid="ignore", over="ignore"):
        rx, ry = c * r.ux - s * r.uy, s * r.ux + c * r.uy                                              # (N, n)
        t = lambda o, j: (o + (j - r.nxy).astype(float) * r.step_xy)[:, None]
        Ca, Cb = _fine(rx + t(r.x, a), r.x0, r.cell, r.sub), _fine(rx + t(r.x, a1), r.x0, r.cell, r.sub)
        Ra, Rb = _fine(ry + t(r.y, b), r.y0, r.cell, r.sub), _fine(ry + t(r.y, b1), r.y0, r.cell, r.sub)
        finite = np.isfinite(Ca) & np.isfinite(Cb) & np.isfinite(Ra) & np.isfinite(Rb)
        outside = (Cb < 0.0) | (Ca >= fw) | (Rb < 0.0) | (Ra >= fh)
        inside = (Ca >= 0.0) & (Ca < fw) & (Ra >= 0.0) & (Ra < fh)
    look = finite & ~outside
    ca = np.where(look, np.maximum(Ca, 0.0), 0.0).astype(np.int64)
    cb = np.where(look, np.minimum(Cb, fw - 1.0), 0.0).astype(np.int64)
    ra = np.where(look, np.maximum(Ra, 0.0), 0.0).astype(np.int64)
    rb = np.where(look, np.minimum(Rb, fh - 1.0), 0.0).astype(np.int64)
    e = np.maximum(cb - ca, rb - ra) + 1
    lvl = np.ceil(np.log2(e)).astype(np.int64)                         # e <= 2^11: exact at powers of two
    assert np.all((1 << lvl) >= e) and np.all((lvl == 0) | ((1 << np.maximum(lvl - 1, 0)) < e))
    built = lvl < r.levels
    term = np.where(look, np.where(built, r.pyr[np.where(built, lvl, 0), ra, ca], 0), np.where(finite, r.cap, 0))
    ri, ci = np.where(inside, Ra, 0.0).astype(np.int64), np.where(inside, Ca, 0.0).astype(np.int64)
    exact = np.where(inside, r.pyr[0][ri, ci], r.cap)
    leaf = ((a == a1) & (b == b1))[:, None]
    return np.where(leaf, exact, term).sum(axis=1, dtype=np.int64)


def _least_square(lo, hi):
    return np.where(lo > 0, lo, np.where(hi < 0, -hi, 0)) ** 2


def node_m_min(r, jth, a, a1, b, b1):
    """the least m = ix^2 + iy^2 + ith^2 of a node's block"""
    jth, a, a1, b, b1 = (np.asarray(v, dtype=np.int64) for v in (jth, a, a1, b, b1))
    return _least_square(a - r.nxy, a1 - r.nxy) + _least_square(b - r.nxy, b1 - r.nxy) + (jth - r.nth) ** 2


def top_nodes(nxy, nth, top_log2):
    """(jth, a, a1, b, b1) of the top-level nodes in the order of their index t = (jth nb + b / 2^h) nb + a / 2^h"""
    nx, side = 2 * nxy + 1, 1 << top_log2
    nb = -(-nx // side)
    jth, by, bx = (v.ravel() for v in np.meshgrid(np.arange(2 * nth + 1), np.arange(nb), np.arange(nb), indexing="ij"))
    a, b = bx * side, by * side
    return jth, a, np.minimum(a + side, nx) - 1, b, np.minimum(b + side, nx) - 1


def top_bound_ref(r, top_log2):
    """top_bound [b] of rmpc_scan_search: int32 (ntop,)"""
    return node_bound_ref(r, *top_nodes(r.nxy, r.nth, top_log2)).astype(np.int32)


# ---- a search on the bound -------------------------------------------------------------------------------------------------
def search_ref(pose, points, ranges, pyr, top_log2, max_range, d2, H, W, sub, cap, x0, y0, cell, nxy, step_xy, nth,
               step_th, rot, min_hits, active=None):
    """Best-first branch and bound: the node of the least key (bound, m_min, 0) is split in four until that key exceeds
    the best leaf's (score, m, k).  Returns match_wide_ref's dict and `leaves` (B,), the candidates scored exactly."""
    pose, points, ranges = (np.asarray(a, dtype=float) for a in (pose, points, ranges))
    geom = dict(max_range=max_range, d2=d2, H=H, W=W, sub=sub, cap=cap, x0=x0, y0=y0, cell=cell, nxy=nxy, step_xy=step_xy,
                nth=nth, step_th=step_th, rot=rot, min_hits=min_hits)
    B, nx = len(pose), 2 * nxy + 1
    out = dict(pose_out=pose[:, :3].copy(), best=np.full(B, -1, np.int32), score=np.zeros(B, np.int32),
               score0=np.zeros(B, np.int32), used=np.zeros(B, np.int32), leaves=np.zeros(B, np.int32))
    for b in range(B):
        r = Robot(pose[b], points[b], ranges[b], pyr, **geom)
        out["used"][b] = len(r.ux)
        if len(r.ux) < min_hits or (active is not None and active[b] == 0):
            continue
        out["score0"][b] = node_bound_ref(r, [nth], [nxy], [nxy], [nxy], [nxy])[0]
        jth, a, a1, bb, b1 = top_nodes(nxy, nth, top_log2)
        v, mm = node_bound_ref(r, jth, a, a1, bb, b1), node_m_min(r, jth, a, a1, bb, b1)
        best, leaves, heap = None, 0, []
        if top_log2 == 0:
            keys = list(zip(v.tolist(), mm.tolist(), ((jth * nx + bb) * nx + a).tolist()))
            best, leaves = min(keys), len(keys)
        else:
            heap = [(int(v[i]), int(mm[i]), 0, int(jth[i]), int(a[i]), int(bb[i]), top_log2) for i in range(len(v))]
            heapq.heapify(heap)
        while heap and (best is None or heap[0][:3] <= best):
            _, _, _, j, a_, b_, h = heapq.heappop(heap)
            half = 1 << (h - 1)
            kids = [(a_ + da, b_ + db) for db in (0, half) for da in (0, half) if a_ + da < nx and b_ + db < nx]
            ka, kb = np.array([k[0] for k in kids]), np.array([k[1] for k in kids])
            ka1, kb1 = np.minimum(ka + half, nx) - 1, np.minimum(kb + half, nx) - 1
            kj = np.full(len(kids), j)
            kv, km = node_bound_ref(r, kj, ka, ka1, kb, kb1), node_m_min(r, kj, ka, ka1, kb, kb1)
            for i in range(len(kids)):
                if h == 1:
                    key = (int(kv[i]), int(km[i]), (j * nx + int(kb[i])) * nx + int(ka[i]))
                    leaves += 1
                    if best is None or key < best:
                        best = key
                elif best is None or (int(kv[i]), int(km[i]), 0) <= best:
                    heapq.heappush(heap, (int(kv[i]), int(km[i]), 0, j, int(ka[i]), int(kb[i]), h - 1))
        k = best[2]
        jth_, jy, jx = k // (nx * nx), (k // nx) % nx, k % nx
        out["best"][b], out["score"][b], out["leaves"][b] = k, best[0], leaves
        out["pose_out"][b] = (r.x + float(jx - nxy) * step_xy, r.y + float(jy - nxy) * step_xy,
                              r.th + float(jth_ - nth) * step_th)
    return out
