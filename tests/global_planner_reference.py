"""The global planner's rules restated on the CPU from the reference (robotmpcs/global_planner/: a_star.py, gridmap.py,
globalPlanner.py).  Rules only: tests/test_global_planner_cpu.py checks them on hand-computed grids,
tests/test_gpu_global_planner.py holds the device against them.
Grids are data[row][col]; a cell index is row * W + col; a move is (dcol, drow) in the reference's order."""
import heapq
import math

import numpy as np

S2 = math.sqrt(2)
MOVES8 = [(1, 0, 1.0), (0, 1, 1.0), (-1, 0, 1.0), (0, -1, 1.0), (1, 1, S2), (-1, 1, S2), (-1, -1, S2), (1, -1, S2)]
MOVES = {8: MOVES8, 4: MOVES8[:4], "8N": MOVES8, "4N": MOVES8[:4]}


def astar_ref(data, start, goal, movement=8, f=3.0, occ=0.8):
    """The reference's heap A* (priority g + h + potential, the potential counted twice); start / goal (x, y) =
    (col, row).  Returns (path [(x, y)], cost = sum of delta + f data over the entered cells), ([], inf) if the goal
    is unreachable; raises as the reference does on occupied end points."""
    H, W = data.shape
    if data[start[1], start[0]] >= occ:
        raise Exception("Start node is not traversable")
    if data[goal[1], goal[0]] >= occ:
        raise Exception("Goal node is not traversable")
    front = [(math.dist(start, goal), 0.0, start, None)]
    came, visited = {}, set()
    pos = None
    while front:
        _, cost, pos, prev = heapq.heappop(front)
        if pos in visited:
            continue
        visited.add(pos)
        came[pos] = (prev, cost)
        if pos == goal:
            break
        for dx, dy, dc in MOVES[movement]:
            n = (pos[0] + dx, pos[1] + dy)
            if not (0 <= n[0] < W and 0 <= n[1] < H) or n in visited or data[n[1], n[0]] >= occ:
                continue
            pot = data[n[1], n[0]] * f
            nc = cost + dc + pot
            heapq.heappush(front, (nc + math.dist(n, goal) + pot, nc, n, pos))
    if pos != goal:
        return [], math.inf
    path, p = [], goal
    while p is not None:
        path.append(p)
        p = came[p][0]
    return path[::-1], came[goal][1]


def field_ref(data, goal_cell, movement=8, f=3.0, occ=0.8):
    """Backward Dijkstra of D(goal) = 0, D(u) = min_v (delta + (f data[v] + D(v))), +inf on occupied cells."""
    H, W = data.shape
    D = np.full(H * W, np.inf)
    gr, gc = divmod(goal_cell, W)
    if not (0 <= goal_cell < H * W) or data[gr, gc] >= occ:
        return D
    D[goal_cell] = 0.0
    heap, done = [(0.0, goal_cell)], np.zeros(H * W, bool)
    while heap:
        d, v = heapq.heappop(heap)
        if done[v]:
            continue
        done[v] = True
        vr, vc = divmod(v, W)
        ev = f * data[vr, vc] + D[v]
        for dx, dy, dc in MOVES[movement]:
            ur, uc = vr - dy, vc - dx           # u + move = v
            if 0 <= ur < H and 0 <= uc < W and data[ur, uc] < occ:
                u = ur * W + uc
                cand = dc + ev
                if cand < D[u]:
                    D[u] = cand
                    heapq.heappush(heap, (cand, u))
    return D.reshape(H, W)


def descend_ref(data, D, start_cell, goal_cell, movement=8, f=3.0):
    """Path down field D: the neighbour with the least delta + (f data[v] + D(v)), the first in move order on ties."""
    H, W = data.shape
    u, path = start_cell, [start_cell]
    while u != goal_cell:
        r, c = divmod(u, W)
        best, nxt = math.inf, -1
        for dx, dy, dc in MOVES[movement]:
            rr, cc = r + dy, c + dx
            if 0 <= rr < H and 0 <= cc < W:
                cand = dc + (f * data[rr, cc] + D[rr, cc])
                if cand < best:
                    best, nxt = cand, rr * W + cc
        u = nxt
        path.append(u)
    return path


def path_cost(data, cells, f=3.0):
    W = data.shape[1]
    cost = 0.0
    for a, b in zip(cells[:-1], cells[1:]):
        (ar, ac), (br, bc) = divmod(a, W), divmod(b, W)
        cost += (1.0 if abs(ar - br) + abs(ac - bc) == 1 else S2) + f * data[br, bc]
    return cost


def inflate_ref(data, cell, size_robot=0.4, threshold=0.29):
    """get_enlarged_obstacles: box mean on the interior, raw values on the border band, then > threshold -> 1."""
    k = int(np.ceil(size_robot / cell))
    kernel = np.ones((2 * k + 1, 2 * k + 1))
    conv = data.copy()
    for i in range(k, data.shape[0] - k):
        for j in range(k, data.shape[1] - k):
            conv[i, j] = np.sum(kernel * data[i - k:i + k + 1, j - k:j + k + 1]) / np.sum(kernel)
    return (conv > threshold).astype(np.float64), conv


class LocalGoalRef:
    """get_local_goal over a path of world points."""

    def __init__(self, threshold=1.3):
        self.idx, self.threshold = 0, threshold

    def __call__(self, position, path):
        d = np.sqrt((path[self.idx][0] - position[0]) ** 2 + (path[self.idx][1] - position[1]) ** 2)
        if self.idx < len(path) - 1 and len(path) > 0 and d <= self.threshold:
            self.idx += 1
        return path[self.idx]
