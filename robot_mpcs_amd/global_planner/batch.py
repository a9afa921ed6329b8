"""The fleet side of the global planner, in the plain frame (cell (row, col) centred at (x0 + col cell, y0 + row cell)):
``plan_batch`` computes one cost-to-go field per distinct goal and one path per query on the device, ``RouteFollower``
keeps the routes on the device and hands every robot its next waypoint once per control step (``get_local_goal`` of
the reference for B robots in one launch) and takes new routes when the map changes (``RouteFollower.replace``,
``replan``), ``shelf_map`` draws a seeded procedural store for tests, the examples and the benchmark, ``store_routes``
enlarges such a map and draws the fleet's (start, goal) cells on it (``pick_routes``)."""
from __future__ import annotations

import numpy as np

from .. import _lib

MOVES = {"8N": 8, "4N": 4, 8: 8, 4: 4}


def _dev_tensor(a, dtype, device):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a, dtype=dtype).to(device).contiguous()


def plan_batch(grid, starts, goal_cells, movement="8N", occupancy_threshold=0.8, occupancy_cost_factor=3.0,
               max_len=None, device=None, stream=None, return_fields=False):
    """grid (H, W) occupancy (numpy or device tensor), starts (B,) and goal_cells (B,) cell indices row * W + col ->
    (paths (B, max_len) int32, lens (B,) int32) on the device; lens as ``rmpc_grid_paths_device`` (> 0 cells, 0
    unreachable, < 0 an error code of ``_lib.GRID_*``).  Each distinct goal gets one field.  max_len defaults to
    4 (H + W), at most H W.  Maps of more than ``_lib.GRID_MAX_CELLS`` cells, up to ``_lib.GRID_LARGE_MAX_CELLS``, take
    ``rmpc_grid_fields_large_device``.  With return_fields, also (fields (G, H, W), status (G,), goal_index (B,))."""
    import torch
    if movement not in MOVES:
        raise ValueError("Unknown movement")
    dev = torch.device(device) if device is not None else (grid.device if torch.is_tensor(grid) else torch.device("cuda", 0))
    g = _dev_tensor(grid, torch.float64, dev)
    H, W = int(g.shape[0]), int(g.shape[1])
    s = _dev_tensor(starts, torch.int32, dev).reshape(-1)
    gc = _dev_tensor(goal_cells, torch.int32, dev).reshape(-1)
    if s.shape[0] != gc.shape[0] or s.shape[0] < 1:
        raise ValueError("starts and goal_cells must both be (B,), B >= 1")
    uniq, inv = torch.unique(gc, return_inverse=True)
    uniq, inv = uniq.to(torch.int32).contiguous(), inv.to(torch.int32).contiguous()
    G = int(uniq.shape[0])
    max_len = int(max_len) if max_len is not None else min(H * W, 4 * (H + W))
    fields = torch.empty((G, H, W), dtype=torch.float64, device=dev)
    status = torch.empty(G, dtype=torch.int32, device=dev)
    paths = torch.empty((s.shape[0], max_len), dtype=torch.int32, device=dev)
    lens = torch.empty(s.shape[0], dtype=torch.int32, device=dev)
    st = _lib.stream_handle(stream, dev)
    # a map beyond one workgroup's LDS takes the tiled entry: the same fields, bit for bit
    fields_device = _lib.grid_fields_large_device if H * W > _lib.GRID_MAX_CELLS else _lib.grid_fields_device
    fields_device(g, uniq, fields, status, MOVES[movement], occupancy_threshold, occupancy_cost_factor, stream=st)
    _lib.grid_paths_device(g, fields, uniq, s, inv, paths, lens, MOVES[movement], occupancy_threshold,
                           occupancy_cost_factor, stream=st)
    if return_fields:
        return paths, lens, (fields, status, inv)
    return paths, lens


def cells_from_positions(pos, H, W, x0, y0, cell, stream=None):
    """pos (B, stride >= 2) device tensor (e.g. xinit) -> cells (B,) int32 of the plain frame, -1 outside."""
    import torch
    cells = torch.empty(pos.shape[0], dtype=torch.int32, device=pos.device)
    _lib.grid_cells_device(pos, cells, H, W, x0, y0, cell, stream=_lib.stream_handle(stream, pos.device))
    return cells


class RouteFollower:
    """Routes of B robots on the device; ``step(xinit, goal)`` is one ``rmpc_follow_path_device`` launch: a robot
    within ``threshold`` of its current waypoint (and not on its last one) moves on to the next, and every robot with a
    route gets its waypoint's centre written into ``goal`` (B, 3) -- the scene's goal array."""

    def __init__(self, paths, lens, W, x0, y0, cell, threshold=1.3):
        import torch
        self.paths, self.lens = paths, lens
        self.idx = torch.zeros(paths.shape[0], dtype=torch.int32, device=paths.device)
        self.W, self.x0, self.y0, self.cell, self.threshold = int(W), float(x0), float(y0), float(cell), float(threshold)

    def step(self, xinit, goal, stream=None):
        _lib.follow_path_device(self.paths, self.lens, self.idx, xinit, goal, self.W, self.x0, self.y0, self.cell,
                                self.threshold, stream=_lib.stream_handle(stream, goal.device))

    def replace(self, paths, lens):
        """New routes (paths (B, max_len) int32, lens (B,) int32, e.g. of ``plan_batch``): the robots with lens > 0 take
        theirs and start at its first cell, the others keep the route and the waypoint they have.  Tensor operations
        only, no host read."""
        import torch
        new = lens > 0
        L = max(int(paths.shape[1]), int(self.paths.shape[1]))
        pad = lambda p: p if p.shape[1] == L else torch.nn.functional.pad(p, (0, L - p.shape[1]))
        self.paths = torch.where(new[:, None], pad(paths), pad(self.paths)).contiguous()
        self.lens = torch.where(new, lens, self.lens)
        self.idx = torch.where(new, torch.zeros_like(self.idx), self.idx)

    def final_goals(self):
        """(B, 2) world centres of the last cell of each route (NaN where a robot has none), on the device."""
        import torch
        L = self.lens.clamp(min=1).long() - 1
        last = self.paths.gather(1, L[:, None])[:, 0].long()
        xy = torch.stack([self.x0 + (last % self.W).double() * self.cell, self.y0 + (last // self.W).double() * self.cell], 1)
        return torch.where((self.lens > 0)[:, None], xy, torch.full_like(xy, float("nan")))


def replan(follower, grid, xinit, goal_cells, **plan_batch_kwargs):
    """Re-routes a fleet on a new map: the robots' current cells (``cells_from_positions`` of xinit (B, stride >= 2)) ->
    ``plan_batch`` on ``grid`` (H, W) to ``goal_cells`` (B,) -> ``follower.replace``.  A robot without a route on the
    new map (its cell or its goal occupied, the goal unreachable, the robot outside the map) keeps the one it has.
    Returns (paths, lens) of the new plan."""
    H, W = int(grid.shape[0]), int(grid.shape[1])
    cells = cells_from_positions(xinit, H, W, follower.x0, follower.y0, follower.cell, stream=plan_batch_kwargs.get("stream"))
    paths, lens = plan_batch(grid, cells, goal_cells, **plan_batch_kwargs)
    follower.replace(paths, lens)
    return paths, lens


def shelf_map(H=41, W=41, seed=0, aisle=4, shelf=2, gap=3, gaps_per_shelf=2):
    """A seeded store: a one-cell outer wall, shelves `shelf` cells deep running along the rows, `aisle` free rows
    between them, a free lane of `aisle` cells at each end (its width varies by one per shelf) and `gaps_per_shelf`
    cross passages `gap` cells wide cut through every shelf.  (H, W) float64, 1 occupied, 0 free."""
    rng = np.random.default_rng(seed)
    g = np.zeros((H, W))
    g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = 1.0
    row = 1 + aisle
    while row + shelf <= H - 1 - aisle:
        left = 1 + aisle + int(rng.integers(0, 2))
        right = W - 1 - aisle - int(rng.integers(0, 2))
        if right - left > 2 * gap:
            g[row:row + shelf, left:right] = 1.0
            for _ in range(gaps_per_shelf):
                c = int(rng.integers(left + gap, max(left + gap + 1, right - 2 * gap)))
                g[row:row + shelf, c:c + gap] = 0.0
        row += shelf + aisle
    return g


def cell_xy(cells, W, x0, y0, cell):
    """(n, 2) centres of the cells (indices row * W + col) in the plain frame"""
    return np.stack([x0 + (cells % W) * cell, y0 + (cells // W) * cell], 1)


def pick_routes(raw, ok, B, rng, x0, y0, cell):
    """B (start, goal) cell pairs among the `ok` cells of the map `raw` (bool, occupied), 10 .. 20 m apart, the straight
    line between them crossing an occupied cell."""
    cells = np.flatnonzero(ok.ravel())
    xy = cell_xy(cells, raw.shape[1], x0, y0, cell)
    starts, goals = [], []
    while len(starts) < B:
        i, j = rng.integers(0, len(cells), 2)
        d = np.linalg.norm(xy[i] - xy[j])
        if not 10.0 <= d <= 20.0:
            continue
        t = np.linspace(0.0, 1.0, 200)[:, None]
        seg = xy[i] + t * (xy[j] - xy[i])
        cc = np.rint((seg - [x0, y0]) / cell).astype(int)
        if not raw[cc[:, 1], cc[:, 0]].any():
            continue
        starts.append(cells[i]); goals.append(cells[j])
    return np.array(starts, np.int32), np.array(goals, np.int32)


def store_routes(raw, B, rng, x0, y0, cell, size_robot, device, ok=None):
    """The prologue of a store example: the map enlarged as the reference does it (``png_values`` through
    ``grid_inflate_device``, box mean > 0.29), then ``pick_routes`` among the cells free on it (below the planner's
    occupancy threshold 0.8) and, if given, in the mask ``ok``.  Returns (g_inf (H, W) on the device, starts, goals);
    ``plan_batch(g_inf, starts, goals)`` and ``RouteFollower`` take it from there."""
    import torch
    from .globalPlanner import png_values   # (globalPlanner imports a_star, which imports this module)
    g_raw = _dev_tensor(png_values(raw), torch.float64, device)
    g_inf = torch.empty_like(g_raw)
    _lib.grid_inflate_device(g_raw, g_inf, cell, size_robot, 0.29)
    free = g_inf.cpu().numpy() < 0.8
    return (g_inf,) + pick_routes(raw > 0.5, free if ok is None else ok & free, B, rng, x0, y0, cell)
