"""Separating planes between the robots of a fleet, built on the device.

Each control step, every robot and every stage of the coming solve gets one plane per nearest neighbour, in the style
of buffered Voronoi cells: both robots of a pair compute the same plane from the same predicted collision points
(robot ``lo`` holds (n, c), robot ``hi`` (-n, -c)), which splits the free gap between them equally.  The planes go
into the scene's ``lin_constrs`` slots, where the LinearConstraints row keeps the collision link r_body from each.
If both robots of a mutual pair keep their new plans on their own sides, the plans stay r_i + r_j apart at every
stage, also when all robots replan at once.

``NeighbourPlanes`` is the counterpart of ``utils.lidar.LidarPlanes``: points -> planes, two launches on one stream
(``rmpc_fleet_points_device``, ``rmpc_fleet_planes_device``).  There is no CPU path.
"""
from __future__ import annotations

from .. import _lib


class NeighbourPlanes:
    """Predicted collision points -> separating planes for B robots with horizon N and K neighbours per stage.

    Owns ``points`` (B, N, 3) and ``planes`` (B, N, nobst, 4) (nobst defaults to slot0 + K), or writes slots
    slot0 .. slot0 + K - 1 of the ``planes`` buffer the caller passes (e.g. one whose other slots hold lidar planes).
    ``range`` (m) bounds the neighbour search: 0 admits nobody (every slot a dummy plane), +inf everyone.
    ``heading`` 1 = the boxer (collision point ``offset`` ahead of the base, at ``height``), 0 = the point robot
    (x, y, height).  ``step`` enqueues the two launches on the current (or the given) stream and never synchronises."""

    def __init__(self, B, N, K, range=float("inf"), heading=1, offset=(0.4, 0.0), height=0.0, slot0=0, nobst=None,
                 planes=None, device=None):
        import torch
        B, N, K, slot0 = int(B), int(N), int(K), int(slot0)
        if B < 1 or N < 1 or not 1 <= K <= 8:
            raise ValueError("NeighbourPlanes: B, N >= 1 and 1 <= K <= 8")
        if int(heading) not in (0, 1):
            raise ValueError("NeighbourPlanes: heading must be 0 or 1")
        if not float(range) >= 0.0:
            raise ValueError("NeighbourPlanes: range must be >= 0")
        if planes is not None:
            nobst = int(planes.shape[2])
            if tuple(planes.shape) != (B, N, nobst, 4) or planes.dtype != torch.float64 or not planes.is_contiguous():
                raise ValueError("NeighbourPlanes: planes must be a contiguous fp64 (B, N, nobst, 4) tensor")
            dev = planes.device
        else:
            nobst = slot0 + K if nobst is None else int(nobst)
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if slot0 < 0 or slot0 + K > nobst:
            raise ValueError("NeighbourPlanes: need 0 <= slot0 and slot0 + K <= nobst")
        self.device = dev
        self.B, self.N, self.K, self.nobst, self.slot0 = B, N, K, nobst, slot0
        self.range, self.heading = float(range), int(heading)
        self.offset, self.height = (float(offset[0]), float(offset[1])), float(height)
        f64 = dict(dtype=torch.float64, device=dev)
        self.points = torch.zeros((B, N, 3), **f64)
        self.planes = planes if planes is not None else torch.zeros((B, N, nobst, 4), **f64)

    def step(self, xinit, r_body, z_prev=None, exitflag=None, stream=None):
        """xinit (B, stride >= 3) poses; r_body (B,) fp64; z_prev (B, N, nvar) the previous plan or None (first step);
        exitflag (B,) int32 or None.  Returns ``planes``."""
        st = _lib.stream_handle(stream, self.device)
        _lib.fleet_points_device(xinit, self.points, z_prev, exitflag, self.heading, self.offset, self.height, stream=st)
        _lib.fleet_planes_device(self.points, r_body, self.planes, self.K, self.range, self.slot0, stream=st)
        return self.planes
