"""The timed routes' rules restated on the CPU from include/rmpc.h (rmpc_timed_plan_device, rmpc_timed_follow_device):
``plan_ref`` works on boolean layers and a reservation table, ``plan_walk`` a cell at a time against the paths already
planned (no table), ``follow_ref`` is the follower's simultaneous step.  tests/test_timed_cpu.py holds the two against
each other and against hand-worked cases, tests/test_gpu_timed.py holds the device against ``plan_ref`` and
``follow_ref`` bit for bit.  Grids are data[row][col]; a cell index is row * W + col; a move is (dcol, drow) in the
planner's order."""
import numpy as np

from global_planner_reference import MOVES, field_ref, inflate_ref

OUTSIDE, BAD_ORDER = -3, -8
INT64_MAX = (1 << 63) - 1


def fields_for(grid, goal_cells, movement, occ=0.8, f=3.0):
    """(Gf, H, W): the field of every goal cell (``field_ref``; +inf everywhere for a goal that is occupied or outside)"""
    H, W = grid.shape
    return np.stack([np.asarray(field_ref(grid, int(g), movement, f, occ), dtype=float).reshape(H, W) for g in goal_cells])


def _skipped(s, gi, HW, Gf):
    return not (0 <= s < HW and 0 <= gi < Gf)


def _d2(a, b, W):
    return (a // W - b // W) ** 2 + (a % W - b % W) ** 2


def _end_cell(cells, D):
    d = np.array([D[c] if D[c] < np.inf else np.inf for c in cells])
    return int(cells[np.lexsort((cells, d))[0]])


def _arrive(p, goal, T):
    a = T + 1
    while a > 0 and p[a - 1] == goal:
        a -= 1
    return a if a <= T else T + 1


def _is_permutation(row, B):
    return sorted(int(v) for v in row) == list(range(B))


def _finish(out, valid, B, T):
    G = len(valid)
    out["key"] = np.full(G, INT64_MAX, dtype=np.int64)
    best = -1
    for g in range(G):
        if not valid[g]:
            continue
        st, ar = out["status"][g], out["arrive"][g]
        key = (int((st > 0).sum()) << 44) | (int((ar > T).sum()) << 32) | int(ar.sum())
        out["key"][g] = key
        if best < 0 or key < out["key"][best]:
            best = g
    out["best"] = np.array([best], dtype=np.int32)
    return out


def _blank(G, B, T):
    return dict(paths=np.full((G, B, T + 1), -1, dtype=np.int32), status=np.full((G, B), BAD_ORDER, dtype=np.int32),
                arrive=np.full((G, B), T + 1, dtype=np.int32))


def plan_ref(grid, start, goal_index, fields, goal_cells, orders, T, sep2, lag=1, movement=4, occ=0.8):
    """The rule of rmpc_timed_plan_device on boolean layers: dict(paths (G, B, T + 1), status, arrive (G, B) int32,
    key (G,) int64, best (1,) int32)."""
    grid = np.asarray(grid, dtype=float)
    H, W = grid.shape
    HW, B, Gf = H * W, len(start), len(fields)
    orders = np.atleast_2d(np.asarray(orders))
    G = orders.shape[0]
    free = ~(grid >= occ)
    rows, cols = np.mgrid[0:H, 0:W]
    disc = lambda c: (rows - c // W) ** 2 + (cols - c % W) ** 2 < sep2
    moves = [(dc, dr) for dc, dr, _ in MOVES[movement]]
    out = _blank(G, B, T)
    valid = [_is_permutation(orders[g], B) for g in range(G)]
    for g in range(G):
        if not valid[g]:
            continue
        res = np.zeros((T + 1, H, W), dtype=bool)
        order = [int(b) for b in orders[g]]
        for k, b in enumerate(order):
            s, gi = int(start[b]), int(goal_index[b])
            if _skipped(s, gi, HW, Gf):
                out["status"][g, b], out["arrive"][g, b] = OUTSIDE, T + 1
                continue
            later = np.zeros((H, W), dtype=bool)
            for j in order[k + 1:]:
                if not _skipped(int(start[j]), int(goal_index[j]), HW, Gf):
                    later |= disc(int(start[j]))
            reach = np.zeros((T + 1, H, W), dtype=bool)
            reach[0, s // W, s % W] = True
            f = 0
            for t in range(1, T + 1):
                pad = np.pad(reach[t - 1], 1)
                n = reach[t - 1].copy()
                for dc, dr in moves:                      # reach[t][c] from reach[t - 1][c - m]
                    n |= pad[1 - dr:1 - dr + H, 1 - dc:1 - dc + W]
                n &= free & ~res[t]
                if t <= lag:
                    n &= ~later
                reach[t] = n
                if not n.any():
                    f = t
                    break
            te = f - 1 if f else T
            end = _end_cell(np.flatnonzero(reach[te].ravel()), np.asarray(fields[gi]).ravel())
            p = np.full(T + 1, end, dtype=np.int32)
            c = end
            for t in range(te, 0, -1):
                r, col = divmod(c, W)
                if not reach[t - 1, r, col]:
                    for dc, dr in moves:
                        rr, cc = r - dr, col - dc
                        if 0 <= rr < H and 0 <= cc < W and reach[t - 1, rr, cc]:
                            c = rr * W + cc
                            break
                p[t - 1] = c
            out["paths"][g, b], out["status"][g, b] = p, f
            out["arrive"][g, b] = _arrive(p, int(goal_cells[gi]), T)
            for t in range(T + 1):
                res[max(0, t - lag):min(T, t + lag) + 1] |= disc(int(p[t]))
    return _finish(out, valid, B, T)


def plan_walk(grid, start, goal_index, fields, goal_cells, orders, T, sep2, lag=1, movement=4, occ=0.8):
    """The same rule a cell at a time: sets of cells, and a cell is reserved at t when it conflicts with a cell that a
    robot planned earlier holds within lag layers of t (no reservation table)."""
    grid = np.asarray(grid, dtype=float)
    H, W = grid.shape
    HW, B, Gf = H * W, len(start), len(fields)
    orders = np.atleast_2d(np.asarray(orders))
    G = orders.shape[0]
    moves = [(dc, dr) for dc, dr, _ in MOVES[movement]]
    out = _blank(G, B, T)
    valid = [_is_permutation(orders[g], B) for g in range(G)]
    for g in range(G):
        if not valid[g]:
            continue
        order, planned = [int(b) for b in orders[g]], []
        for k, b in enumerate(order):
            s, gi = int(start[b]), int(goal_index[b])
            if _skipped(s, gi, HW, Gf):
                out["status"][g, b] = OUTSIDE
                continue
            later = [int(start[j]) for j in order[k + 1:] if not _skipped(int(start[j]), int(goal_index[j]), HW, Gf)]

            def admitted(c, t):
                r, col = divmod(c, W)
                if grid[r, col] >= occ:
                    return False
                if t <= lag and any(_d2(c, sj, W) < sep2 for sj in later):
                    return False
                for q in planned:
                    for u in range(max(0, t - lag), min(T, t + lag) + 1):
                        if _d2(c, int(q[u]), W) < sep2:
                            return False
                return True

            reach, f = [{s}], 0
            for t in range(1, T + 1):
                cand = set()
                for c in reach[t - 1]:
                    r, col = divmod(c, W)
                    cand.add(c)
                    for dc, dr in moves:
                        if 0 <= r + dr < H and 0 <= col + dc < W:
                            cand.add((r + dr) * W + col + dc)
                layer = {c for c in cand if admitted(c, t)}
                reach.append(layer)
                if not layer:
                    f = t
                    break
            te = f - 1 if f else T
            end = _end_cell(np.array(sorted(reach[te])), np.asarray(fields[gi]).ravel())
            p = [end] * (T + 1)
            c = end
            for t in range(te, 0, -1):
                if c not in reach[t - 1]:
                    r, col = divmod(c, W)
                    for dc, dr in moves:
                        rr, cc = r - dr, col - dc
                        if 0 <= rr < H and 0 <= cc < W and rr * W + cc in reach[t - 1]:
                            c = rr * W + cc
                            break
                p[t - 1] = c
            out["paths"][g, b], out["status"][g, b] = p, f
            out["arrive"][g, b] = _arrive(p, int(goal_cells[gi]), T)
            planned.append(p)
    return _finish(out, valid, B, T)


def conflicts(paths, status, W, sep2, lag):
    """the (i, j, t, s) with i < j, both of status 0, |s - t| <= lag and d2(p_i[t], p_j[s]) < sep2 -- the guarantee
    says there are none"""
    paths = np.asarray(paths, dtype=np.int64)
    ok = [b for b in range(len(paths)) if status[b] == 0]
    T = paths.shape[1] - 1
    r, c = paths // W, paths % W
    bad = []
    for a, i in enumerate(ok):
        for j in ok[a + 1:]:
            for k in range(-lag, lag + 1):
                t = np.arange(max(0, -k), min(T, T - k) + 1)
                d2 = (r[i, t] - r[j, t + k]) ** 2 + (c[i, t] - c[j, t + k]) ** 2
                bad += [(i, j, int(tt), int(tt + k)) for tt in t[d2 < sep2]]
    return bad


def follow_ref(paths, idx_in, pos, goal, W, x0, y0, cell, threshold, sep2, lag=1):
    """One step of rmpc_timed_follow_device: (idx_out, goal, blocked); pos (B, >= 2), goal (B, 3) is copied."""
    paths = np.asarray(paths)
    B, T = paths.shape[0], paths.shape[1] - 1
    idx_out, blocked, goal = np.array(idx_in, dtype=np.int32), np.full(B, -1, dtype=np.int32), np.array(goal, dtype=float)
    centre = lambda c: (x0 + float(c % W) * cell, y0 + float(c // W) * cell)
    for b in range(B):
        p = paths[b]
        if p[0] < 0:
            continue
        i = min(max(int(idx_in[b]), 0), T)
        cx, cy = centre(int(p[i]))
        dx, dy = cx - pos[b, 0], cy - pos[b, 1]
        if i < T and np.sqrt(dx * dx + dy * dy) <= threshold:
            for j in range(B):
                if j == b or paths[j, 0] < 0:
                    continue
                if any(_d2(int(paths[j, s]), int(p[i + 1]), W) < sep2 and not int(idx_in[j]) >= s + lag
                       for s in range(0, i - lag + 1)):
                    blocked[b] = j
                    break
            if blocked[b] < 0:
                i += 1
        idx_out[b] = i
        goal[b] = centre(int(p[i])) + (0.0,)
    return idx_out, goal, blocked


# ---- the store case ----------------------------------------------------------------------------------------------------
def store_grid(seed=0):
    """(raw, g_inf): the store's true map and the planning grid the store examples make of it (``store_routes``:
    ``png_values``, then the box mean > 0.29 at k = ceil(size_robot / cell))"""
    from robot_mpcs_amd.global_planner import png_values
    from robot_mpcs_amd.store import STORE, store_map
    raw = store_map(seed)
    return raw, inflate_ref(png_values(raw), STORE.cell, STORE.size_robot, 0.29)[0]


def store_case(B=16, seed=0, sep2=9):
    """(raw, g_inf, starts, goals): B routes of ``pick_routes`` among the cells ``clear_cells(raw, 2)`` that the planning
    grid calls free, drawn by ``pick_spaced_routes`` from ``default_rng(seed)``: starts pairwise at least sep2 (squared
    cells) apart, goals too"""
    from robot_mpcs_amd.global_planner import pick_spaced_routes
    from robot_mpcs_amd.store import STORE, clear_cells
    raw, g_inf = store_grid(seed)
    ok = clear_cells(raw, STORE.clear_cells) & (g_inf < 0.8)
    starts, goals = pick_spaced_routes(raw > 0.5, ok, B, np.random.default_rng(seed), STORE.x0, STORE.y0, STORE.cell, sep2)
    return raw, g_inf, starts, goals
