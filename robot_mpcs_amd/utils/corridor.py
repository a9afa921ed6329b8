"""Safe corridors from the map, built on the device (include/rmpc_corridor.h).

Each control step, every robot and every stage of the coming solve gets one rectangle of cells known to be free,
grown round the cell of the predicted collision point, and its four faces as half-planes in the scene's
``lin_constrs`` slots, where the LinearConstraints row keeps the collision link r_body from each.  The static world
becomes a constraint of the MPC without a sensor model: the map itself is read, through the summed-area table of its
occupancy, and a rectangle excludes every occupied cell by construction.

``MapCorridors`` is the counterpart of ``utils.lidar.LidarPlanes`` and ``utils.separation.NeighbourPlanes``: points ->
planes, two launches on one stream (``rmpc_fleet_points_device``, ``rmpc_grid_corridor_device``).  There is no CPU path.
"""
from __future__ import annotations

from .. import _lib


class MapCorridors:
    """Predicted collision points -> corridor planes for B robots with horizon N on the map ``grid`` (H, W) fp64 whose
    cell (row, col) has its centre at (x0 + col cell, y0 + row cell); a cell is occupied when its value is not below
    ``occupancy_threshold``.

    Owns ``sums`` (H + 1, W + 1) int32, ``points`` (B, N, 3), ``rects`` (B, N, 4) int32 (r0, r1, c0, c1), ``status``
    (B, N) int32 (1 a corridor, 0 the point's cell is occupied, -1 the point is outside the map or not finite; <= 0:
    dummy planes) and ``planes`` (B, N, nobst, 4) (nobst defaults to slot0 + 4), or writes slots slot0 .. slot0 + 3 of
    the ``planes`` buffer the caller passes (e.g. one whose other slots ``NeighbourPlanes`` writes).  ``reach``: the most
    cells a face lies from the point's cell.  ``heading`` 1 = the boxer (collision point ``offset`` ahead of the base, at
    ``height``), 0 = the point robot (x, y, height).  ``set_grid`` rebuilds the sums for a changed map (one call, two
    launches); ``step`` enqueues its two launches on the current (or the given) stream and never synchronises."""

    def __init__(self, B, N, grid, x0, y0, cell, occupancy_threshold=0.8, reach=8, heading=0, offset=(0, 0), height=0.0,
                 slot0=0, nobst=None, planes=None, device=None):
        import torch
        B, N, slot0, reach = int(B), int(N), int(slot0), int(reach)
        if B < 1 or N < 1 or not 1 <= reach <= _lib.CORRIDOR_MAX_REACH:
            raise ValueError("MapCorridors: B, N >= 1 and 1 <= reach <= %d" % _lib.CORRIDOR_MAX_REACH)
        if int(heading) not in (0, 1):
            raise ValueError("MapCorridors: heading must be 0 or 1")
        if planes is not None:
            nobst = int(planes.shape[2])
            if tuple(planes.shape) != (B, N, nobst, 4) or planes.dtype != torch.float64 or not planes.is_contiguous():
                raise ValueError("MapCorridors: planes must be a contiguous fp64 (B, N, nobst, 4) tensor")
        else:
            nobst = slot0 + 4 if nobst is None else int(nobst)
        if slot0 < 0 or slot0 + 4 > nobst:
            raise ValueError("MapCorridors: need 0 <= slot0 and slot0 + 4 <= nobst")
        if planes is not None:
            dev = planes.device
        else:
            dev = torch.device(device) if device is not None else (
                grid.device if grid.is_cuda else torch.device("cuda", torch.cuda.current_device()))
        self.device = dev
        self.B, self.N, self.nobst, self.slot0, self.reach = B, N, nobst, slot0, reach
        self.x0, self.y0, self.cell = float(x0), float(y0), float(cell)
        self.occupancy_threshold, self.heading = float(occupancy_threshold), int(heading)
        self.offset, self.height = (float(offset[0]), float(offset[1])), float(height)
        self.H, self.W = int(grid.shape[0]), int(grid.shape[1])
        i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
        self.sums = torch.zeros((self.H + 1, self.W + 1), **i32)
        self.points = torch.zeros((B, N, 3), **f64)
        self.rects = torch.full((B, N, 4), -1, **i32)
        self.status = torch.zeros((B, N), **i32)
        self.planes = planes if planes is not None else torch.zeros((B, N, nobst, 4), **f64)
        self.set_grid(grid)

    def set_grid(self, grid, stream=None):
        """The map changed (``FleetMap.occupancy``): rebuild the sums from ``grid`` (H, W) fp64 of the shape given at
        construction."""
        import torch
        if tuple(grid.shape) != (self.H, self.W) or grid.dtype != torch.float64:
            raise ValueError("MapCorridors: grid must be an fp64 (%d, %d) tensor" % (self.H, self.W))
        grid = grid.to(self.device).contiguous()
        _lib.grid_occ_sums_device(grid, self.sums, self.occupancy_threshold, stream=_lib.stream_handle(stream, self.device))

    def step(self, xinit, z_prev=None, exitflag=None, stream=None):
        """xinit (B, stride >= 3) poses; z_prev (B, N, nvar) the previous plan or None (first step); exitflag (B,) int32
        or None.  Returns ``planes``."""
        st = _lib.stream_handle(stream, self.device)
        _lib.fleet_points_device(xinit, self.points, z_prev, exitflag, self.heading, self.offset, self.height, stream=st)
        _lib.grid_corridor_device(self.sums, self.points, self.planes, self.x0, self.y0, self.cell, self.reach, self.slot0,
                                  rect=self.rects, status=self.status, stream=st)
        return self.planes
