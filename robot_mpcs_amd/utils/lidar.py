"""The lidar preprocessing of the reference's boxer examples on the device, for a fleet.

``examples/boxer_example_supermarket.py`` turns a lidar scan into a point cloud (``compute_point_cloud``), then runs the
free-space decomposition once per stage around the sensor position of that stage in the previous plan, and hands the
planes to ``setLinearConstraints``; its comment asks for "a preprocessor class".  ``LidarPlanes`` is that class for
B robots: scan -> plan points -> FSD, three launches on one stream (``rmpc_lidar_scan_device``,
``rmpc_plan_points_device``, ``rmpc_free_space_device``), writing the ``lin_constrs`` array a scene points at.
``boxes_from_grid`` turns an occupancy map into the boxes the scan sees, so that the lidar and the global planner see
one world.  With ``body_radius`` the scan also sees the fleet's own robots (``rmpc_lidar_scan_fleet_device``).  There is
no CPU path.
"""
from __future__ import annotations

import math

import numpy as np

from .. import _lib


def boxes_from_grid(raw, x0, y0, cell):
    """(nbox, 4) boxes (cx, cy, lx, ly) whose union is exactly the occupied cells (value > 0.5) of ``raw`` [row][col],
    each cell a square of side ``cell`` centred at (x0 + col cell, y0 + row cell): maximal runs per row, then identical
    runs of consecutive rows joined into one box."""
    occ = np.asarray(raw) > 0.5
    H, W = occ.shape
    spans = []                 # (row0, row1, col0, col1), inclusive
    open_runs = {}             # (col0, col1) -> first row of the box that run continues
    for r in range(H + 1):
        runs = []
        if r < H:
            row = np.concatenate(([False], occ[r], [False])).astype(np.int8)
            edges = np.flatnonzero(np.diff(row))
            runs = [(int(a), int(b) - 1) for a, b in zip(edges[0::2], edges[1::2])]
        cont = {}
        for run in runs:
            cont[run] = open_runs.pop(run, r)
        for (c0, c1), r0 in open_runs.items():
            spans.append((r0, r - 1, c0, c1))
        open_runs = cont
    spans.sort()
    out = np.zeros((len(spans), 4))
    for n, (r0, r1, c0, c1) in enumerate(spans):
        out[n] = (x0 + 0.5 * (c0 + c1) * cell, y0 + 0.5 * (r0 + r1) * cell, (c1 - c0 + 1) * cell, (r1 - r0 + 1) * cell)
    return out


class LidarPlanes:
    """Scan -> per-stage seeds -> free-space decomposition for B robots with horizon N and K planes per stage.

    Owns the buffers: ``points`` (B, rays, 3), ``ranges`` (B, rays), ``seeds`` (B, N, 3) and ``planes`` (B, N, K, 4),
    the array a scene's ``lin_constrs`` points at.  ``step(xinit, z_prev, exitflag)`` enqueues the three launches on the
    current (or the given) stream and never synchronises.  The defaults are the boxer's: the sensor 0.4 m ahead of the
    base at height 0.02, ``max_radius`` 5 (the reference's FreeSpaceDecomposition), a full circle of 64 rays (the
    FSD kernel takes at most 64 points).

    With ``body_radius`` (a scalar or (B,)) the robots see each other: the block's own robots are round
    bodies of that radius centred at ``body_offset`` in the body frame (default: the sensor offset; ``heading`` = 0
    for a robot without one, whose body sits at (x, y)), robot b being body b.  ``step`` then takes the centres from
    the poses (``rmpc_fleet_points_device``, N = 1, into ``centres`` (B, 1, 3)) and runs the fleet scan
    (``rmpc_lidar_scan_fleet_device``) into ``owner`` (B, rays) int32 and ``static_ranges`` (B, rays) as well: four
    launches.  ``step(..., bodies=(centres, radius, self0))`` scans those bodies instead (other blocks' robots, a mixed
    fleet), with or without ``body_radius``."""

    def __init__(self, B, N, K, boxes=None, circles=None, rays=64, angle_min=-math.pi, angle_max=math.pi, max_range=10.0,
                 max_radius=5.0, offset=(0.4, 0.0), height=0.02, device=None, body_radius=None, body_offset=None,
                 heading=1):
        import torch
        if not 1 <= int(rays) <= 64:
            raise ValueError("LidarPlanes: 1 <= rays <= 64 (the free-space decomposition reads at most 64 points)")
        if int(B) < 1 or int(N) < 1 or int(K) < 1:
            raise ValueError("LidarPlanes: B, N, K >= 1")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        f64 = dict(dtype=torch.float64, device=dev)
        shape = lambda a, w: torch.as_tensor(np.zeros((0, w)) if a is None else a, dtype=torch.float64).reshape(-1, w) \
            .to(dev).contiguous()
        self.device = dev
        self.B, self.N, self.K, self.rays = int(B), int(N), int(K), int(rays)
        self.boxes, self.circles = shape(boxes, 4), shape(circles, 3)
        self.angle_min, self.angle_max, self.max_range = float(angle_min), float(angle_max), float(max_range)
        self.max_radius, self.offset, self.height = float(max_radius), (float(offset[0]), float(offset[1])), float(height)
        self.points = torch.zeros((self.B, self.rays, 3), **f64)
        self.ranges = torch.zeros((self.B, self.rays), **f64)
        self.seeds = torch.zeros((self.B, self.N, 3), **f64)
        self.planes = torch.zeros((self.B, self.N, self.K, 4), **f64)
        self.body_radius = self.centres = self.owner = self.static_ranges = None
        self.heading = int(heading)
        self.body_offset = self.offset if body_offset is None else (float(body_offset[0]), float(body_offset[1]))
        if body_radius is not None:
            self.body_radius = torch.as_tensor(body_radius, dtype=torch.float64).reshape(-1).to(dev).expand(self.B) \
                .contiguous()
            self.centres = torch.zeros((self.B, 1, 3), **f64)
            self._fleet_buffers()

    def _fleet_buffers(self):
        import torch
        self.owner = torch.zeros((self.B, self.rays), dtype=torch.int32, device=self.device)
        self.static_ranges = torch.zeros((self.B, self.rays), dtype=torch.float64, device=self.device)

    def _scan_fleet(self, xinit, bodies, st):
        if self.owner is None:          # bodies handed to a block built without body_radius: on their first use
            self._fleet_buffers()
        if bodies is None:
            _lib.fleet_points_device(xinit, self.centres, None, None, self.heading, self.body_offset, 0.0, stream=st)
            bodies = (self.centres, self.body_radius, 0)
        centres, radius, self0 = bodies
        _lib.lidar_scan_fleet_device(xinit, self.points, centres, radius, self.boxes, self.circles, self.angle_min,
                                     self.angle_max, self.max_range, self.offset, self.height, self0=self0,
                                     owner=self.owner, static_ranges=self.static_ranges, ranges=self.ranges, stream=st)

    def step(self, xinit, z_prev=None, exitflag=None, stream=None, bodies=None):
        """xinit (B, stride >= 3) poses; z_prev (B, N, nvar) the previous plan or None (first step); exitflag (B,) int32
        or None; bodies (centres (P, stride >= 2) or (P, 1, 3), radius (P,), self0) device tensors or None.  Returns
        ``planes``."""
        st = _lib.stream_handle(stream, self.device)
        if bodies is not None or self.body_radius is not None:
            self._scan_fleet(xinit, bodies, st)
        else:
            _lib.lidar_scan_device(xinit, self.points, self.boxes, self.circles, self.angle_min, self.angle_max,
                                   self.max_range, self.offset, self.height, ranges=self.ranges, stream=st)
        _lib.plan_points_device(xinit, self.seeds, z_prev, exitflag, self.offset, self.height, stream=st)
        _lib.free_space_decomposition_device(self.points, self.seeds, self.planes, self.max_radius, stream=st)
        return self.planes
