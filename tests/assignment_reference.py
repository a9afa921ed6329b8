"""The rules of coordinated exploration (include/rmpc.h: rmpc_grid_targets_device, rmpc_grid_route_costs_device,
rmpc_assign_greedy_device) restated in numpy.  Rules only: tests/test_assignment_cpu.py checks them on
hand-computed cases and one restatement against the other, tests/test_gpu_assignment.py holds the device against them."""
import math

import numpy as np

from global_planner_reference import MOVES

INF = math.inf


def tiles_of(H, W, tile):
    return -(-H // tile) * -(-W // tile)


def targets_ref(seed, tile):
    """rmpc_grid_targets_device: (target_cells (T,) int32, tseeds (T, H, W)); Python integers, which do not overflow"""
    H, W = seed.shape
    ntc = -(-W // tile)
    T = tiles_of(H, W, tile)
    members = [[] for _ in range(T)]
    for r in range(H):
        for c in range(W):
            if seed[r, c] < INF:
                members[(r // tile) * ntc + c // tile].append((r, c))
    targets = np.full(T, -1, dtype=np.int32)
    tseeds = np.full((T, H, W), INF)
    for t, cells in enumerate(members):
        if not cells:
            continue
        n, Sr, Sc = len(cells), sum(r for r, _ in cells), sum(c for _, c in cells)
        _, cell = min(((n * r - Sr) ** 2 + (n * c - Sc) ** 2, r * W + c) for r, c in cells)
        targets[t] = cell
        tseeds[t].ravel()[cell] = 0.0
    return targets, tseeds


def route_costs_ref(data, fields, start_cells, movement=8, f=3.0, occ=0.8):
    """rmpc_grid_route_costs_device: cost (B, T)"""
    H, W = data.shape
    B, T = len(start_cells), len(fields)
    cost = np.full((B, T), INF)
    for b, u in enumerate(start_cells):
        if not 0 <= u < H * W:
            continue
        r, c = divmod(int(u), W)
        for t in range(T):
            D = fields[t]
            if D[r, c] < INF:
                cost[b, t] = D[r, c]
                continue
            best = INF
            for dx, dy, dc in MOVES[movement]:
                rr, cc = r + dy, c + dx
                if 0 <= rr < H and 0 <= cc < W and data[rr, cc] < occ:
                    cand = dc + (f * data[rr, cc] + D[rr, cc])
                    if cand < best:
                        best = cand
            cost[b, t] = best
    return cost


def takeable_of(cost):
    with np.errstate(invalid="ignore"):
        return (cost >= 0.0) & (cost < INF)


def greedy_ref(cost):
    """rmpc_assign_greedy_device, the sequential rule as written: (assign (B,), passes (B,)), passes counted from 0.
    argmin over the row-major matrix returns the first of equal costs: the least (b, t)."""
    cost = np.asarray(cost, dtype=float)
    B, T = cost.shape
    ok = takeable_of(cost)
    assign, passes = np.full(B, -1, dtype=np.int32), np.full(B, -1, dtype=np.int32)
    free = np.ones(B, dtype=bool)
    p = 0
    while True:
        avail = np.ones(T, dtype=bool)
        took = 0
        while avail.any():
            m = ok & free[:, None] & avail[None, :]
            if not m.any():
                break
            b, t = divmod(int(np.argmin(np.where(m, cost, INF))), T)
            assign[b], passes[b], free[b], avail[t] = t, p, False, False
            took += 1
        if took == 0 or not free.any():
            return assign, passes
        p += 1


def greedy_sorted_ref(cost):
    """The same rule by another road, for the large cases: per pass the takeable pairs of the free robots are sorted by
    (cost, b, t) (a stable sort of the row-major order) and swept once; a pair whose robot and target are both still
    there is taken, which is what the sequential rule does, since taking a pair only ever removes later pairs."""
    cost = np.asarray(cost, dtype=float)
    B, T = cost.shape
    ok = takeable_of(cost)
    assign, passes = np.full(B, -1, dtype=np.int32), np.full(B, -1, dtype=np.int32)
    free = np.ones(B, dtype=bool)
    p = 0
    while True:
        rows = np.flatnonzero(free)
        sub, subok = cost[rows], ok[rows]
        idx = np.flatnonzero(subok.ravel())
        order = idx[np.argsort(sub.ravel()[idx] + 0.0, kind="stable")]
        avail = np.ones(T, dtype=bool)
        left = int(subok.any(axis=0).sum())          # targets that can still be taken in this pass, at most
        took = 0
        for k in order.tolist():
            if left == 0:
                break
            i, t = divmod(k, T)
            b = rows[i]
            if free[b] and avail[t]:
                assign[b], passes[b], free[b], avail[t] = t, p, False, False
                took += 1
                left -= 1
        if took == 0 or not free.any():
            return assign, passes
        p += 1
