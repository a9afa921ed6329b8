"""The corridors of include/rmpc_corridor.h restated on the CPU, written from the header: ``occ_sums_ref`` (a numpy
cumsum), ``corridor_ref`` (plain loops over (b, k) on the summed-area table, the doubles formed in the header's order)
and ``corridor_plain``, a second restatement that tests a new line by slicing the boolean occupancy instead of the
table.  ``grow`` / ``grow_plain`` are the rectangle of one seed cell with the number of rounds it took."""
import numpy as np


def occupancy(grid, thr):
    """the any-angle rule !(v < thr): a NaN is occupied"""
    return ~(np.asarray(grid, dtype=np.float64) < thr)


def occ_sums_ref(grid, thr):
    """S (H + 1, W + 1) int32: row 0 and column 0 are 0, S[r + 1, c + 1] counts the occupied cells of rows 0..r, columns 0..c"""
    occ = occupancy(grid, thr)
    S = np.zeros((occ.shape[0] + 1, occ.shape[1] + 1), dtype=np.int32)
    S[1:, 1:] = occ.astype(np.int32).cumsum(0).cumsum(1)
    return S


def count(S, ra, rb, ca, cb):
    return int(S[rb + 1, cb + 1]) - int(S[ra, cb + 1]) - int(S[rb + 1, ca]) + int(S[ra, ca])


def grow(S, r, c, reach):
    """((r0, r1, c0, c1), rounds) from the free seed cell (r, c), the line counts from the table"""
    H, W = S.shape[0] - 1, S.shape[1] - 1
    return _grow(H, W, r, c, reach, lambda ra, rb, ca, cb: count(S, ra, rb, ca, cb) == 0)


def grow_plain(occ, r, c, reach):
    """the same from the boolean occupancy, written apart: the rectangle as [lo, hi] per axis, a direction as (axis,
    sign), the new line tested by slicing the occupancy padded with an occupied rim (so the map's edge is a line like
    any other)"""
    H, W = occ.shape
    pad = np.ones((H + 2, W + 2), dtype=bool)
    pad[1:-1, 1:-1] = occ
    lo, hi, seed = [r, c], [r, c], (r, c)             # axis 0 the rows, axis 1 the columns
    rounds = 0
    while True:
        rounds += 1
        before = (tuple(lo), tuple(hi))
        for axis, sign in ((1, +1), (0, +1), (1, -1), (0, -1)):
            line = (hi if sign > 0 else lo)[axis] + sign
            if abs(line - seed[axis]) > reach:
                continue
            span = [slice(lo[0] + 1, hi[0] + 2), slice(lo[1] + 1, hi[1] + 2)]
            span[axis] = slice(line + 1, line + 2)
            if pad[span[0], span[1]].any():
                continue
            (hi if sign > 0 else lo)[axis] = line
        if before == (tuple(lo), tuple(hi)):
            return (lo[0], hi[0], lo[1], hi[1]), rounds


def _grow(H, W, r, c, reach, free):
    r0 = r1 = r
    c0 = c1 = c
    rounds = 0
    while True:
        rounds += 1
        advanced = False
        if c1 + 1 < W and c1 + 1 - c <= reach and free(r0, r1, c1 + 1, c1 + 1):
            c1, advanced = c1 + 1, True
        if r1 + 1 < H and r1 + 1 - r <= reach and free(r1 + 1, r1 + 1, c0, c1):
            r1, advanced = r1 + 1, True
        if c0 - 1 >= 0 and c - (c0 - 1) <= reach and free(r0, r1, c0 - 1, c0 - 1):
            c0, advanced = c0 - 1, True
        if r0 - 1 >= 0 and r - (r0 - 1) <= reach and free(r0 - 1, r0 - 1, c0, c1):
            r0, advanced = r0 - 1, True
        if not advanced:
            return (r0, r1, c0, c1), rounds


def seed_cell(p, H, W, x0, y0, cell):
    """(r, c) as rmpc_grid_cells_device forms a cell (rint: half to even), None outside the map or not finite"""
    with np.errstate(invalid="ignore", over="ignore"):
        fc, fr = np.rint((np.float64(p[0]) - x0) / cell), np.rint((np.float64(p[1]) - y0) / cell)
    if fc >= 0.0 and fc < W and fr >= 0.0 and fr < H:
        return int(fr), int(fc)
    return None


def face_planes(rect, x0, y0, cell):
    """(4, 4) fp64: the header's planes of (r0, r1, c0, c1), every operation in its order"""
    r0, r1, c0, c1 = rect
    x0, y0, cell = np.float64(x0), np.float64(y0), np.float64(cell)
    xlo, xhi = x0 + (np.float64(c0) - 0.5) * cell, x0 + (np.float64(c1) + 0.5) * cell
    ylo, yhi = y0 + (np.float64(r0) - 0.5) * cell, y0 + (np.float64(r1) + 0.5) * cell
    return np.array([[1.0, 0.0, 0.0, -xlo], [-1.0, 0.0, 0.0, xhi], [0.0, 1.0, 0.0, -ylo], [0.0, -1.0, 0.0, yhi]])


def dummy_plane(s):
    """the free-space decomposition's dummy plane around the point s: HalfPlane(s + (20, 20, 0), s)"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(s, dtype=np.float64)
        q = s + np.array([20.0, 20.0, 0.0])
        n = s - q
        return np.array([n[0], n[1], n[2], -((n[0] * q[0] + n[1] * q[1]) + n[2] * q[2])])


def _corridors(points, planes, slot0, x0, y0, cell, H, W, occupied, rectangle):
    B, N = points.shape[:2]
    rect = np.full((B, N, 4), -1, dtype=np.int32)
    status = np.zeros((B, N), dtype=np.int32)
    for b in range(B):
        for k in range(N):
            s = seed_cell(points[b, k], H, W, x0, y0, cell)
            status[b, k] = -1 if s is None else (0 if occupied(*s) else 1)
            if status[b, k] == 1:
                rect[b, k] = rectangle(*s)
                planes[b, k, slot0:slot0 + 4] = face_planes(rect[b, k], x0, y0, cell)
            else:
                planes[b, k, slot0:slot0 + 4] = dummy_plane(points[b, k])
    return rect, status


def corridor_ref(S, x0, y0, cell, points, reach, planes, slot0):
    """rmpc_grid_corridor_device on the table S: writes slots slot0 .. slot0 + 3 of planes (B, N, nobst, 4) in place and
    returns (rect (B, N, 4) int32, status (B, N) int32)"""
    H, W = S.shape[0] - 1, S.shape[1] - 1
    return _corridors(points, planes, slot0, x0, y0, cell, H, W, lambda r, c: count(S, r, r, c, c) != 0,
                      lambda r, c: grow(S, r, c, reach)[0])


def corridor_plain(occ, x0, y0, cell, points, reach, planes, slot0):
    """the same from the boolean occupancy"""
    H, W = occ.shape
    return _corridors(points, planes, slot0, x0, y0, cell, H, W, lambda r, c: bool(occ[r, c]),
                      lambda r, c: grow_plain(occ, r, c, reach)[0])


def canonical_bits(a):
    """the uint64 view of fp64 values with every NaN as one pattern: which NaN an operation on infinities yields (its
    sign, its payload) is the processor's choice, not the rule's"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))
