"""The fleet's map from its own lidar scans, on the device: ``FleetMap`` keeps two int32 grids of evidence in the global
planner's plain frame (cell (row, col) centred at (x0 + col cell, y0 + row cell)) -- how often a ray ended in a cell
(``hits``) and how often one crossed it (``misses``) -- and classifies them into the occupancy grid that
``grid_inflate_device`` and ``plan_batch`` read (``rmpc_grid_mark_device``, ``rmpc_grid_occupancy_device``;
DESIGN.md 14).  The reference gets its map from a simulator's ground truth; a fleet that carries lidars builds it from
what it sees.  There is no CPU path.
"""
from __future__ import annotations

from .. import _lib


class FleetMap:
    """Evidence and occupancy grid (H, W) of B robots with ``rays`` rays each.

    Owns ``hits``, ``misses`` (H, W) int32, ``origins`` (B, 1, 3), ``skipped`` (1,) int32 and ``grid`` (H, W) fp64.
    ``max_range``, ``offset`` and ``height`` are the scan's (``LidarPlanes``).  ``hit_depth``: how far behind a hit's
    end point its cell is taken; the end point lies on the obstacle's face, in a world from ``boxes_from_grid`` a cell
    edge.  With 0.01 cell the numpy restatement marks 60 - 180 occupied corner cells as crossed per 16 k - 32 k rays (a
    ray that grazes a corner enters the cell beside it), with 1e-6 m none."""

    def __init__(self, B, H, W, x0, y0, cell, rays, max_range, offset, height, hit_depth=1e-6, w_hit=3, w_miss=1,
                 device=None):
        import torch
        if int(B) < 1 or int(rays) < 1 or int(H) < 1 or int(W) < 1:
            raise ValueError("FleetMap: B, rays, H, W >= 1")
        if int(H) * int(W) > _lib.GRID_MAX_CELLS:
            raise ValueError(f"FleetMap: at most {_lib.GRID_MAX_CELLS} cells")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.B, self.H, self.W, self.rays = int(B), int(H), int(W), int(rays)
        self.x0, self.y0, self.cell = float(x0), float(y0), float(cell)
        self.max_range, self.offset, self.height = float(max_range), (float(offset[0]), float(offset[1])), float(height)
        self.hit_depth, self.w_hit, self.w_miss = float(hit_depth), int(w_hit), int(w_miss)
        self.hits = torch.zeros((self.H, self.W), dtype=torch.int32, device=dev)
        self.misses = torch.zeros((self.H, self.W), dtype=torch.int32, device=dev)
        self.skipped = torch.zeros(1, dtype=torch.int32, device=dev)
        self.origins = torch.zeros((self.B, 1, 3), dtype=torch.float64, device=dev)
        self.grid = torch.zeros((self.H, self.W), dtype=torch.float64, device=dev)

    def mark(self, xinit, points, ranges, stream=None):
        """xinit (B, stride >= 3) the poses the scan was taken from, points (B, rays, 3) and ranges (B, rays) the scan
        (``LidarPlanes.points``, ``LidarPlanes.ranges``): two launches on the current (or the given) stream, the sensor
        origins and the marks; never synchronises."""
        st = _lib.stream_handle(stream, self.device)
        _lib.plan_points_device(xinit, self.origins, None, None, self.offset, self.height, stream=st)
        _lib.grid_mark_device(self.origins, points, ranges, self.hits, self.misses, self.x0, self.y0, self.cell,
                              self.max_range, self.hit_depth, skipped=self.skipped, stream=st)

    def occupancy(self, free_value, occ_value, unknown_value, forget=0, stream=None):
        """Classifies the evidence into ``grid`` (returned) and, with forget > 0, ages the counters."""
        _lib.grid_occupancy_device(self.hits, self.misses, self.grid, free_value, occ_value, unknown_value, self.w_hit,
                                   self.w_miss, forget, stream=_lib.stream_handle(stream, self.device))
        return self.grid

    def reset(self):
        """Zeroes the evidence (and the count of skipped rays)."""
        self.hits.zero_()
        self.misses.zero_()
        self.skipped.zero_()
