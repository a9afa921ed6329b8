"""The rules of frontier exploration (include/rmpc.h: rmpc_grid_frontier_device, rmpc_grid_fields_seeded_device,
rmpc_grid_descend_device) restated in numpy.  Rules only: tests/test_exploration_cpu.py checks them on
hand-computed cases and in a kinematic exploration, tests/test_gpu_exploration.py holds the device against them."""
import heapq
import math

import numpy as np

from global_planner_reference import MOVES, MOVES8

INF = math.inf
OK, OUTSIDE, TOO_LONG, BAD_MAP, BAD_SEED = 0, -3, -4, -5, -7


def frontier_ref(hits, misses, enlarged, occ=0.8, nmoves=4, unknown_value=1.0):
    """rmpc_grid_frontier_device: (plan (H, W), seed (H, W), count)"""
    known = (np.asarray(hits).astype(np.int64) + np.asarray(misses).astype(np.int64)) != 0
    H, W = known.shape
    plan = np.where(known, enlarged, unknown_value)
    unknown = np.pad(~known, 1, constant_values=False)          # the map's edge is not unknown
    beside = np.zeros((H, W), dtype=bool)
    for dx, dy, _ in MOVES8[:nmoves]:
        beside |= unknown[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    frontier = known & (np.asarray(enlarged) < occ) & beside
    return plan, np.where(frontier, 0.0, INF), int(frontier.sum())


def field_seeded_ref(data, seeds, movement=8, f=3.0, occ=0.8):
    """rmpc_grid_fields_seeded_device for one field, a heap Dijkstra from every finite seed on a free cell:
    D(u) = min(seed(u), min_v (delta + (f data[v] + D(v)))), +inf on occupied cells.  Returns (D (H, W), status)."""
    H, W = data.shape
    free = data < occ
    if (free & ~(data >= 0.0)).any():
        return np.full((H, W), INF), BAD_MAP
    s = np.where(free, seeds, INF)
    if (~(s >= 0.0)).any():
        return np.full((H, W), INF), BAD_SEED
    D = s.astype(float).ravel().copy()
    heap = [(D[c], int(c)) for c in np.flatnonzero(np.isfinite(D))]
    heapq.heapify(heap)
    done = np.zeros(H * W, bool)
    while heap:
        d, v = heapq.heappop(heap)
        if done[v]:
            continue
        done[v] = True
        vr, vc = divmod(v, W)
        ev = f * data[vr, vc] + D[v]
        for dx, dy, dc in MOVES[movement]:
            ur, uc = vr - dy, vc - dx           # u + move = v
            if 0 <= ur < H and 0 <= uc < W and free[ur, uc]:
                u = ur * W + uc
                cand = dc + ev
                if cand < D[u]:
                    D[u] = cand
                    heapq.heappush(heap, (cand, u))
    return D.reshape(H, W), OK


def descend_seeded_ref(data, D, seeds, start_cell, movement=8, f=3.0, occ=0.8, max_len=None):
    """rmpc_grid_descend_device for one robot: (cells written, len)"""
    H, W = data.shape
    max_len = H * W if max_len is None else max_len
    if not 0 <= start_cell < H * W:
        return [], OUTSIDE
    Df, Sf = D.ravel(), np.asarray(seeds).ravel()
    u, path = int(start_cell), []
    while True:
        if len(path) >= max_len:
            return path, TOO_LONG
        source = Df[u] < INF and Df[u] == Sf[u]
        nxt = -1
        if not source:
            r, c = divmod(u, W)
            best = INF
            for dx, dy, dc in MOVES[movement]:
                rr, cc = r + dy, c + dx
                if 0 <= rr < H and 0 <= cc < W and data[rr, cc] < occ:
                    cand = dc + (f * data[rr, cc] + D[rr, cc])
                    if cand < best:
                        best, nxt = cand, rr * W + cc
            if nxt < 0:
                return [], 0
        path.append(u)
        if source:
            return path, len(path)
        u = nxt
