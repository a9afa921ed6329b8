"""The rule of include/rmpc_any_angle.h restated on the CPU: the integer cell walk (``touched``, ``visible_walk``), the
greedy shortener (``shorten_ref``) and one step of the follower that looks ahead (``follow_visible_ref``), in plain
Python integers and numpy doubles; and a second, plain statement of line of sight that knows nothing of the walk
(``visible_plain``: exact rationals, every closed unit square of the bounding box against the closed segment).
tests/test_any_angle_cpu.py holds the two against each other and pins hand-worked cases,
tests/test_gpu_any_angle.py holds the device against the walk, bit for bit.
Grids are data[row][col]; a cell index is row * W + col."""
from fractions import Fraction

import numpy as np

OUTSIDE, TOO_LONG = -3, -4         # RMPC_GRID_OUTSIDE, RMPC_GRID_TOO_LONG (include/rmpc.h)


def occupancy(data, occ=0.8):
    """rows of bools: the planner's test, a NaN is occupied"""
    return (~(np.asarray(data, dtype=np.float64) < occ)).tolist()


def touched(r0, c0, r1, c1):
    """the cells the header's walk tests from (r0, c0) to (r1, c1), in its order: every cell whose closed square meets
    the closed segment between the centres, the first one apart"""
    dx, dy = abs(c1 - c0), abs(r1 - r0)
    sx, sy = (1 if c1 >= c0 else -1), (1 if r1 >= r0 else -1)
    e, n, r, c = dx - dy, dx + dy, r0, c0
    dx, dy = 2 * dx, 2 * dy
    while n > 0:
        if e > 0:
            c, e, n = c + sx, e - dy, n - 1
        elif e < 0:
            r, e, n = r + sy, e + dx, n - 1
        else:
            yield r, c + sx
            yield r + sy, c
            r, c, e, n = r + sy, c + sx, e + dx - dy, n - 2
        yield r, c


def visible_walk(occ, W, a, b):
    """occ: ``occupancy`` of the map; a, b cells inside it"""
    for r, c in touched(a // W, a % W, b // W, b % W):
        if occ[r][c]:
            return False
    return True


def _meets(r0, c0, r1, c1, r, c):
    """does the closed segment between the centres of (r0, c0) and (r1, c1) meet the closed unit square of (r, c)?  The
    parameters t in [0, 1] whose point lies in the square's column band and in its row band, intersected."""
    t0, t1 = Fraction(0), Fraction(1)
    for a, d, m in ((c0, c1 - c0, c), (r0, r1 - r0, r)):
        lo, hi = Fraction(2 * m - 1, 2) - a, Fraction(2 * m + 1, 2) - a
        if d == 0:
            if not lo <= 0 <= hi:
                return False
        else:
            u, v = sorted((lo / d, hi / d))
            t0, t1 = max(t0, u), min(t1, v)
    return t0 <= t1


def visible_plain(occ, W, a, b):
    r0, c0, r1, c1 = a // W, a % W, b // W, b % W
    for r in range(min(r0, r1), max(r0, r1) + 1):
        for c in range(min(c0, c1), max(c0, c1) + 1):
            if (r, c) != (r0, c0) and occ[r][c] and _meets(r0, c0, r1, c1, r, c):
                return False
    return True


def visible_pairs_ref(data, a, b, occ=0.8):
    """what rmpc_grid_visible_device writes: 1, 0, or -1 for a cell outside the map"""
    H, W = data.shape
    o = occupancy(data, occ)
    out = np.empty(len(a), dtype=np.int32)
    for t, (x, y) in enumerate(zip(np.asarray(a).tolist(), np.asarray(b).tolist())):
        out[t] = -1 if not (0 <= x < H * W and 0 <= y < H * W) else int(visible_walk(o, W, x, y))
    return out


def shorten_path(o, W, p, reach=0, keep=None):
    """one valid path p (a list of cells) -> (kept cells, their indices in p)"""
    L = len(p)
    out, src, i = [p[0]], [0], 0
    while i < L - 1:
        hi = min(L - 1, i + (reach if reach else L - 1))
        if keep is not None:
            hi = min([hi] + [k for k in range(i + 1, hi + 1) if keep[k] != 0][:1])
        j = hi
        while j > i + 1 and not visible_walk(o, W, p[i], p[j]):
            j -= 1
        out.append(p[j])
        src.append(j)
        i = j
    return out, src


def shorten_ref(data, paths, lens, reach=0, keep=None, occ=0.8, fill=-9):
    """what rmpc_grid_shorten_device leaves in (out, out_len, src) that held ``fill`` everywhere before the call"""
    H, W = data.shape
    o = occupancy(data, occ)
    B, max_len = paths.shape
    out, src = np.full((B, max_len), fill, dtype=np.int32), np.full((B, max_len), fill, dtype=np.int32)
    out_len = np.full(B, fill, dtype=np.int32)
    for b in range(B):
        L = int(lens[b])
        if L <= 0 or L > max_len:
            out_len[b] = L if L <= 0 else TOO_LONG
            continue
        p = paths[b, :L].tolist()
        if not all(0 <= c < H * W for c in p):
            out_len[b] = OUTSIDE
            continue
        cells, idx = shorten_path(o, W, p, reach, None if keep is None else keep[b, :L].tolist())
        out_len[b] = len(cells)
        out[b, :len(cells)], src[b, :len(cells)] = cells, idx
    return out, out_len, src


def chain_length(cells, W, cell):
    """the Euclidean length of a chain of cells, by the formula of ``route_lengths``"""
    c = np.asarray(cells, dtype=np.int64)
    r, q = (c // W).astype(np.float64), (c % W).astype(np.float64)
    return float(np.sqrt((r[1:] - r[:-1]) ** 2 + (q[1:] - q[:-1]) ** 2).sum() * cell)


def _col_row(c, W):
    """c % W and c / W as C forms them (truncation: a cell below 0 keeps its sign)"""
    q = abs(c) // W * (1 if c >= 0 else -1)
    return c - q * W, q


def follow_visible_ref(data, paths, lens, idx, pos, x0, y0, cell, reach, look_ahead, goal, blocked, occ=0.8):
    """one call of rmpc_follow_visible_device: idx, goal (B, 3) and blocked (B,) are updated in place"""
    H, W = data.shape
    o = occupancy(data, occ)
    f8 = np.float64
    x0, y0, cell, look_ahead = f8(x0), f8(y0), f8(cell), f8(look_ahead)
    for b in range(paths.shape[0]):
        L = int(lens[b])
        if L <= 0:
            continue
        p = paths[b]
        i = min(max(int(idx[b]), 0), L - 1)
        px, py = f8(pos[b, 0]), f8(pos[b, 1])
        with np.errstate(invalid="ignore"):
            fc, fr = np.rint((px - x0) / cell), np.rint((py - y0) / cell)
        inside = bool(fc >= 0.0 and fc < W and fr >= 0.0 and fr < H)
        j, found = i, False
        if inside:
            s = int(fr) * W + int(fc)
            for k in range(min(L - 1, i + reach), i - 1, -1):
                c = int(p[k])
                col, row = _col_row(c, W)
                cx, cy = x0 + f8(col) * cell, y0 + f8(row) * cell
                dx, dy = cx - px, cy - py
                if 0 <= c < H * W and np.sqrt(dx * dx + dy * dy) <= look_ahead and visible_walk(o, W, s, c):
                    j, found = k, True
                    break
        col, row = _col_row(int(p[j]), W)
        idx[b] = j
        goal[b] = (x0 + f8(col) * cell, y0 + f8(row) * cell, 0.0)
        blocked[b] = 0 if found else 1
