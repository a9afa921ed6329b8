"""Any-angle routes (include/rmpc_any_angle.h): ``visible`` answers whether one cell of a grid is in line
of sight of another, ``shorten_routes`` pulls the dense 8-connected routes of ``plan_batch`` tight by it (a greedy
string pull, not an optimal any-angle path), ``route_lengths`` measures a chain of cells, and ``VisibleFollower`` is a
``RouteFollower`` whose look-ahead goal is the farthest route cell the robot can see.  Everything runs on the device
and nothing here reads a device value on the host."""
from __future__ import annotations

from .. import _lib
from .batch import RouteFollower, _dev_tensor


def visible(grid, a, b, occupancy_threshold=0.8, stream=None):
    """grid (H, W) fp64 device tensor, a and b (P,) cells row * W + col -> (P,) int32 on the device: 1 where b is in
    line of sight of a (no cell the closed segment between the centres touches, a apart, is occupied), 0 where not,
    -1 for a cell outside the map."""
    import torch
    a = _dev_tensor(a, torch.int32, grid.device).reshape(-1)
    b = _dev_tensor(b, torch.int32, grid.device).reshape(-1)
    if a.shape != b.shape or a.shape[0] < 1:
        raise ValueError("a and b must both be (P,), P >= 1")
    out = torch.empty(a.shape[0], dtype=torch.int32, device=grid.device)
    _lib.grid_visible_device(grid, a, b, out, occupancy_threshold, stream=_lib.stream_handle(stream, grid.device))
    return out


def shorten_routes(grid, paths, lens, reach=0, keep=None, occupancy_threshold=0.8, stream=None):
    """paths (B, max_len) int32, lens (B,) int32 of ``plan_batch`` on grid (H, W) -> (paths, lens, src) of the same
    layout: from every kept cell the next one is the farthest cell of the route, at most ``reach`` cells on (0: any),
    that is in line of sight, or the route's own next cell.  keep (B, max_len) int32 or None: cells that are never
    skipped (a tour's stops).  src holds the index in the input of every kept cell, -1 past the end; cells past the
    new length are 0.  ``RouteFollower``, ``replace`` and ``final_goals`` take the result as it is."""
    import torch
    H, W = int(grid.shape[0]), int(grid.shape[1])
    out, src = torch.zeros_like(paths), torch.full_like(paths, -1)
    out_len = torch.empty_like(lens)
    work = torch.empty(_lib.shorten_work_bytes(H, W) // 4, dtype=torch.int32, device=grid.device)
    _lib.grid_shorten_device(grid, paths, lens, out, out_len, work, reach=reach, keep=keep, src=src,
                             occ_threshold=occupancy_threshold, stream=_lib.stream_handle(stream, grid.device))
    return out, out_len, src


def route_lengths(paths, lens, W, cell):
    """(B,) fp64 on the device: the Euclidean length in metres of each chain of cells, 0 for a robot without a route."""
    import torch
    r, c = (paths // W).double(), (paths % W).double()
    seg = ((r[:, 1:] - r[:, :-1]) ** 2 + (c[:, 1:] - c[:, :-1]) ** 2).sqrt()
    k = torch.arange(1, paths.shape[1], device=paths.device)
    return (seg * (k[None, :] < lens[:, None])).sum(dim=1) * float(cell)


class VisibleFollower(RouteFollower):
    """A ``RouteFollower`` that looks: ``step(xinit, goal)`` is one ``rmpc_follow_visible_device`` launch, after which
    every robot's waypoint is the farthest cell of its route, at most ``reach`` cells on and ``look_ahead`` metres away,
    that its own cell sees on ``grid``; ``blocked`` (B,) int32 is 1 where no cell qualified (the robot is outside the
    map or sees nothing of its route): the hook for a re-plan.  ``set_grid`` takes a map that changed."""

    def __init__(self, paths, lens, W, x0, y0, cell, grid, reach=16, look_ahead=1.3, occupancy_threshold=0.8):
        import torch
        super().__init__(paths, lens, W, x0, y0, cell, threshold=look_ahead)
        self.reach, self.look_ahead, self.occupancy_threshold = int(reach), float(look_ahead), float(occupancy_threshold)
        self.blocked = torch.zeros(paths.shape[0], dtype=torch.int32, device=paths.device)
        self.set_grid(grid)

    def set_grid(self, grid):
        if int(grid.shape[1]) != self.W:
            raise ValueError("the grid's width is not the follower's")
        self.grid = grid.contiguous()

    def step(self, xinit, goal, stream=None):
        _lib.follow_visible_device(self.paths, self.lens, self.idx, xinit, goal, self.grid, self.x0, self.y0, self.cell,
                                   reach=self.reach, look_ahead=self.look_ahead, blocked=self.blocked,
                                   occ_threshold=self.occupancy_threshold, stream=_lib.stream_handle(stream, goal.device))
