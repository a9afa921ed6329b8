"""The traffic-aware routes restated on the CPU from include/rmpc_traffic.h.  Rules only: tests/test_traffic_cpu.py checks
them on hand-computed cases and against each other, tests/test_gpu_traffic.py holds the device against them.

Two restatements of the field: ``field_ref`` iterates the header's recursion D(u) = min_m (c(u, m) + D(u + m)) over whole
arrays until nothing changes (the fixed point as the header defines it), ``field_heap`` is a plain heap Dijkstra on the
directed graph, run backwards from the goal.  A flow table is flow [9][H][W] int32, a cell index row * W + col, a move
(dcol, drow) in the header's order."""
import heapq

import numpy as np

INF = 2 ** 31 - 1
MOVES = [(1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1)]
OPP = [2, 3, 0, 1, 6, 7, 4, 5]
OK, START_OCCUPIED, GOAL_OCCUPIED, OUTSIDE, TOO_LONG = 0, -1, -2, -3, -4          # RMPC_GRID_* of rmpc.h
MAX_EDGE = 65535


def make_costs(base_axial=1000, base_diag=1414, w_visit=300, cap_visit=32, w_contra=700, cap_contra=15):
    return dict(base_axial=base_axial, base_diag=base_diag, w_visit=w_visit, cap_visit=cap_visit, w_contra=w_contra,
                cap_contra=cap_contra)


def refused(k):
    """the header's rule for a rmpc_traffic_costs that is refused"""
    return (k["base_axial"] < 1 or k["base_diag"] < 1 or min(k["w_visit"], k["cap_visit"], k["w_contra"], k["cap_contra"]) < 0
            or k["cap_visit"] > 255 or k["cap_contra"] > 15
            or max(k["base_axial"], k["base_diag"]) + k["w_visit"] * k["cap_visit"] + k["w_contra"] * k["cap_contra"] > MAX_EDGE)


def base(k, m):
    return k["base_axial"] if m < 4 else k["base_diag"]


def free_cells(grid, occ):
    with np.errstate(invalid="ignore"):
        return grid < occ                      # a NaN is occupied


def empty_flow(H, W):
    return np.zeros((9, H, W), np.int32)


def add_ref(flow, paths, lens, sign=1, select=None):
    """rmpc_grid_traffic_add_device, in place on flow [9][H][W]"""
    _, H, W = flow.shape
    max_len = paths.shape[1]
    for b in range(paths.shape[0]):
        if lens[b] <= 0 or (select is not None and select[b] == 0):
            continue
        n = min(int(lens[b]), max_len)
        for j in range(n):
            u = int(paths[b, j])
            if not 0 <= u < H * W:
                continue
            flow[8, u // W, u % W] += sign
            if j + 1 < n:
                v = int(paths[b, j + 1])
                if 0 <= v < H * W:
                    d = (v % W - u % W, v // W - u // W)
                    if d in MOVES:
                        flow[MOVES.index(d), u // W, u % W] += sign
    return flow


def count_routes(H, W, routes):
    """the table of a list of routes (lists of cells), counted afresh"""
    flow = empty_flow(H, W)
    for p in routes:
        if len(p):
            add_ref(flow, np.array([p], np.int64), np.array([len(p)]))
    return flow


def entered_cost(flow, k, m):
    """[H][W] int64: what the header adds to base_m for a step by move m that *enters* the cell: the visits of the cell
    and the routes that leave it by opp(m)"""
    vis = np.minimum(np.maximum(flow[8].astype(np.int64), 0), k["cap_visit"])
    con = np.minimum(np.maximum(flow[OPP[m]].astype(np.int64), 0), k["cap_contra"])
    return k["w_visit"] * vis + k["w_contra"] * con


def edge_cost(flow, k, u, m, W):
    """c(u, m) of the header for the cell index u; u + m must be inside the map"""
    v = u + MOVES[m][1] * W + MOVES[m][0]
    vis = min(max(int(flow[8].flat[v]), 0), k["cap_visit"])
    con = min(max(int(flow[OPP[m]].flat[v]), 0), k["cap_contra"])
    return base(k, m) + k["w_visit"] * vis + k["w_contra"] * con


def shifted(a, dc, dr, fill):
    """b [r][c] = a [r + dr][c + dc] where that is inside the map, ``fill`` elsewhere"""
    H, W = a.shape
    b = np.full_like(a, fill)
    rs, cs = slice(max(0, -dr), min(H, H - dr)), slice(max(0, -dc), min(W, W - dc))
    rd, cd = slice(max(0, dr), min(H, H + dr)), slice(max(0, dc), min(W, W + dc))
    b[rs, cs] = a[rd, cd]
    return b


def field_status(grid, occ, goal):
    H, W = grid.shape
    if not 0 <= goal < H * W:
        return OUTSIDE
    return OK if free_cells(grid, occ).flat[goal] else GOAL_OCCUPIED


def field_ref(grid, occ, flow, k, goal, movement=8):
    """(D [H][W] int32, status): the header's recursion iterated on whole arrays from D(goal) = 0, INF elsewhere, until a
    pass changes nothing"""
    H, W = grid.shape
    D = np.full((H, W), INF, np.int64)
    st = field_status(grid, occ, goal)
    if st != OK:
        return D.astype(np.int32), st
    free = free_cells(grid, occ)
    D.flat[goal] = 0
    step = [shifted(entered_cost(flow, k, m), *MOVES[m], 0) + base(k, m) for m in range(movement)]
    for _ in range(H * W + 1):
        new = D.copy()
        for m in range(movement):
            Dv = shifted(D, *MOVES[m], INF)
            new = np.minimum(new, np.where(Dv < INF, Dv + step[m], INF))
        new[~free] = INF
        new.flat[goal] = 0
        if np.array_equal(new, D):
            break
        D = new
    return D.astype(np.int32), OK


def field_heap(grid, occ, flow, k, goal, movement=8):
    """the same values by a plain heap Dijkstra, backwards from the goal over the edges u -> v = u + m of cost c(u, m)"""
    H, W = grid.shape
    D = np.full(H * W, INF, np.int64)
    st = field_status(grid, occ, goal)
    if st != OK:
        return D.reshape(H, W).astype(np.int32), st
    free = free_cells(grid, occ).ravel()
    D[goal] = 0
    heap, done = [(0, goal)], np.zeros(H * W, bool)
    while heap:
        d, v = heapq.heappop(heap)
        if done[v]:
            continue
        done[v] = True
        vr, vc = divmod(v, W)
        for m in range(movement):
            ur, uc = vr - MOVES[m][1], vc - MOVES[m][0]                 # u + m = v
            if 0 <= ur < H and 0 <= uc < W and free[ur * W + uc]:
                u = ur * W + uc
                cand = d + edge_cost(flow, k, u, m, W)
                if cand < D[u]:
                    D[u] = cand
                    heapq.heappush(heap, (cand, u))
    return D.reshape(H, W).astype(np.int32), OK


def descend_ref(grid, occ, flow, k, D, start, goal, movement=8, max_len=None):
    """(cells, len) as rmpc_grid_paths_traffic_device reports them: len > 0 with its cells, else 0 or an error code with
    no cells"""
    H, W = grid.shape
    max_len = H * W if max_len is None else max_len
    if not (0 <= start < H * W and 0 <= goal < H * W):
        return [], OUTSIDE
    free = free_cells(grid, occ).ravel()
    if not free[start]:
        return [], START_OCCUPIED
    if not free[goal]:
        return [], GOAL_OCCUPIED
    if D.flat[start] == INF:
        return [], 0
    u, path = start, []
    while True:
        if len(path) >= max_len:
            return [], TOO_LONG
        path.append(u)
        if u == goal:
            return path, len(path)
        r, c = divmod(u, W)
        best, nxt = INF, -1
        for m in range(movement):
            rr, cc = r + MOVES[m][1], c + MOVES[m][0]
            if 0 <= rr < H and 0 <= cc < W and D[rr, cc] != INF:
                cand = edge_cost(flow, k, u, m, W) + int(D[rr, cc])
                if cand < best:
                    best, nxt = cand, rr * W + cc
        if nxt < 0:
            return [], 0
        u = nxt


def score_ref(flow, base_axial, base_diag):
    """(L, V, C) of rmpc_grid_traffic_score_device, Python integers"""
    f = flow.astype(np.int64)
    L = sum((base_axial if m < 4 else base_diag) * int(f[m].sum()) for m in range(8))
    V = int((f[8] * (f[8] - 1) // 2).sum())
    C = sum(int((f[m] * shifted(f[OPP[m]], *MOVES[m], 0)).sum()) for m in (0, 1, 4, 5))
    return L, V, C


def route_cost(flow, k, cells, W):
    """the cost of a route under a table: the sum of its steps' c(u, m)"""
    cost = 0
    for u, v in zip(cells[:-1], cells[1:]):
        m = MOVES.index((v % W - u % W, v // W - u // W))
        cost += edge_cost(flow, k, u, m, W)
    return cost


def plan_ref(grid, occ, k, starts, goals, movement=8, groups=1, rounds=2, max_len=None, on_step=None):
    """``TrafficRoutes.plan`` restated: (routes: a list of cell lists, lens, flow, scores [rounds + 1][3]).
    ``on_step(b_list, old routes, new routes, flow of the others)`` is called after every group's step."""
    H, W = grid.shape
    B = len(starts)
    max_len = min(H * W, 4 * (H + W)) if max_len is None else max_len

    def route(bs, flow):
        fields = {g: field_ref(grid, occ, flow, k, g, movement)[0] for g in sorted({int(goals[b]) for b in bs})}
        return [descend_ref(grid, occ, flow, k, fields[int(goals[b])], int(starts[b]), int(goals[b]), movement, max_len) for b in bs]

    def as_arrays(rs):
        p = np.zeros((len(rs), max_len), np.int64)
        for i, r in enumerate(rs):
            p[i, :len(r)] = r
        return p

    flow = empty_flow(H, W)
    routes, lens = map(list, zip(*route(range(B), flow)))
    add_ref(flow, as_arrays(routes), np.array(lens))
    scores = [score_ref(flow, k["base_axial"], k["base_diag"])]
    for _ in range(rounds):
        for j in range(groups):
            bs = list(range(j, B, groups))
            old = [routes[b] for b in bs]
            add_ref(flow, as_arrays(old), np.array([lens[b] for b in bs]), -1)
            new = route(bs, flow)
            if on_step is not None:
                on_step(bs, old, [n[0] for n in new], flow.copy())
            for b, (r, n) in zip(bs, new):
                routes[b], lens[b] = r, n
            add_ref(flow, as_arrays([n[0] for n in new]), np.array([n[1] for n in new]))
        scores.append(score_ref(flow, k["base_axial"], k["base_diag"]))
    return routes, np.array(lens, np.int32), flow, np.array(scores, np.int64)
