"""The work-list rule of the large-map fields (include/rmpc_grid_large.h, csrc/rmpc_grid_large.hpp)
restated in numpy.  Rules only: tests/test_grid_large_cpu.py holds the restatement against the heap Dijkstras
(global_planner_reference.field_ref, exploration_reference.field_seeded_ref), tests/test_gpu_grid_large.py holds the
device against both, visit counts included.

The map is cut into tiles of tile x tile cells (edge tiles smaller), tile index (r // tile) * ceil(W / tile) + c // tile.
A visit of a tile clears its key, relaxes its cells in place against the one-cell ring around it (held constant) until a
sweep lowers nothing, and wakes every neighbouring tile beside which it lowered a cell: the neighbour's key becomes the
least of its key and the new D of those lowered cells.  A tile is active while its key is finite.  A source counts as a
cell lowered from +inf to its seed: the tiles that hold a source and the tiles a source lies beside start active, with
the least such seed as their key (0 for a goal)."""
import heapq
import math

import numpy as np

from global_planner_reference import MOVES

INF = math.inf
ORDERS = ("zigzag", "least")


def serpentine(H, W):
    """every other row a wall with one gap, at alternating ends: one corridor through the whole map"""
    g = np.zeros((H, W))
    for k, r in enumerate(range(1, H, 2)):
        g[r, :] = 1.0
        g[r, W - 1 if k % 2 == 0 else 0] = 0.0
    return g


def tiled_field_ref(data, source, tile, movement=8, order="least", f=3.0, occ=0.8):
    """source: a goal cell (int) or a seed grid (H, W).  order "zigzag": passes over the tiles, ascending index on
    even passes and descending on odd ones, every tile visited that is active when it is reached; "least": the active
    tile with the least (key, index) next.  Returns (D (H, W), visits); the inputs are those the entries accept (free
    cells >= 0, seeds >= 0, the goal free)."""
    if order not in ORDERS:
        raise ValueError("order")
    data = np.asarray(data, dtype=np.float64)
    H, W = data.shape
    T = int(tile)
    nty, ntx = -(-H // T), -(-W // T)
    free = data < occ
    D = np.full((H + 2, W + 2), INF)                       # the map inside a ring of +inf
    if np.ndim(source) == 0:
        if 0 <= int(source) < H * W and free.ravel()[int(source)]:
            D[1 + int(source) // W, 1 + int(source) % W] = 0.0
    else:
        D[1:-1, 1:-1] = np.where(free, np.asarray(source, dtype=np.float64), INF)
    Fr = np.zeros((H + 2, W + 2), bool)
    Fr[1:-1, 1:-1] = free
    P = np.zeros((H + 2, W + 2))
    P[1:-1, 1:-1] = np.where(free, data, 0.0)
    key = np.full(nty * ntx, INF)
    moves = MOVES[movement]

    def wake(ty, tx, low, new, itself=False):
        """the tiles beside which tile (ty, tx) lowered a cell (low, new: the tile's mask and values) take the least of
        those values as their key"""
        h, w = low.shape
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dy == 0 and dx == 0 and not itself) or (movement == 4 and dy != 0 and dx != 0):
                    continue
                if not (0 <= ty + dy < nty and 0 <= tx + dx < ntx):
                    continue
                rows = slice(None) if dy == 0 else (slice(0, 1) if dy < 0 else slice(h - 1, h))
                cols = slice(None) if dx == 0 else (slice(0, 1) if dx < 0 else slice(w - 1, w))
                m = low[rows, cols]
                if m.any():
                    nb = (ty + dy) * ntx + tx + dx
                    key[nb] = min(key[nb], new[rows, cols][m].min())

    # a source is a cell lowered from +inf to its seed: its tile and the tiles it lies beside start active
    for ty in range(nty):
        for tx in range(ntx):
            first = D[1 + ty * T:1 + min(H, ty * T + T), 1 + tx * T:1 + min(W, tx * T + T)]
            wake(ty, tx, first < INF, first, itself=True)

    def visit(t):
        ty, tx = divmod(t, ntx)
        r0, r1, c0, c1 = ty * T, min(H, ty * T + T), tx * T, min(W, tx * T + T)
        key[t] = INF
        h, w = r1 - r0, c1 - c0
        L = D[r0:r1 + 2, c0:c1 + 2].copy()                 # the tile and its ring
        fr, p = Fr[r0:r1 + 2, c0:c1 + 2], P[r0:r1 + 2, c0:c1 + 2]
        old = L[1:-1, 1:-1].copy()
        # the tile's local fixed point (unique, so any fair order finds it): a heap Dijkstra from every finite cell of
        # the tile and the ring, which lowers the tile's free cells only
        Ll, frl, pl = L.tolist(), fr.tolist(), p.tolist()
        heap = [(Ll[i][j], i, j) for i, j in zip(*(a.tolist() for a in np.nonzero(np.isfinite(L) & fr)))]
        heapq.heapify(heap)
        while heap:
            d, i, j = heapq.heappop(heap)
            if d > Ll[i][j]:
                continue
            ev = f * pl[i][j] + d
            for dx, dy, dc in moves:
                ui, uj = i - dy, j - dx                    # u + move = v
                if 1 <= ui <= h and 1 <= uj <= w and frl[ui][uj]:
                    cand = dc + ev
                    if cand < Ll[ui][uj]:
                        Ll[ui][uj] = cand
                        heapq.heappush(heap, (cand, ui, uj))
        new = np.array(Ll)[1:-1, 1:-1]
        D[r0 + 1:r1 + 1, c0 + 1:c1 + 1] = new
        wake(ty, tx, new < old, new)

    visits = 0
    if order == "zigzag":
        p = 0
        while np.isfinite(key).any():
            for t in (range(nty * ntx) if p % 2 == 0 else range(nty * ntx - 1, -1, -1)):
                if key[t] < INF:
                    visit(t)
                    visits += 1
            p += 1
    else:
        while True:
            t = int(np.argmin(key))                        # the first of the least: the least (key, index)
            if not key[t] < INF:
                break
            visit(t)
            visits += 1
    return D[1:-1, 1:-1].copy(), visits
