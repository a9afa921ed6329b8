"""Where a robot believes it is: ``ScanMatcher`` corrects a pose prior by correlative scan matching of the robot's own
lidar ranges against a map (``rmpc_grid_edge_distance_device``, ``rmpc_lidar_project_device``,
``rmpc_scan_match_device``), and ``OdometryDrift`` is the wheel odometry that makes the prior drift.  The
other fleet features read the pose off the simulator's state; a robot on a shop floor has these two.  ``ScanSearcher``
finds the matcher's pose over a window of metres instead of centimetres, for a robot whose estimate is lost
(``rmpc_grid_min_pyramid_device``, ``rmpc_scan_search_device``).  There is no CPU path for the matcher or
the searcher; the odometry is plain torch element-wise arithmetic.
"""
from __future__ import annotations

import numpy as np

from .. import _lib


def rotation_table(nth: int, step_th: float):
    """(2 nth + 1, 2) fp64: (cos, sin) of (j - nth) step_th, the ``rot`` of ``rmpc_scan_match`` -- computed on the host,
    so that the device and a numpy restatement that shares it agree bit for bit"""
    a = (np.arange(2 * int(nth) + 1, dtype=np.float64) - float(nth)) * float(step_th)
    return np.stack([np.cos(a), np.sin(a)], axis=1)


class ScanMatcher:
    """Scan matching for B robots on a map (H, W) in the planner's plain frame, against a lattice of
    (2 nxy + 1)^2 (2 nth + 1) poses at ``step_xy`` [m] and ``step_th`` [rad] around the prior.

    Owns ``d2`` (H sub, W sub) int32, ``rot`` (2 nth + 1, 2), ``points`` (B, rays, 3), ``pose_out`` (B, 3) and ``best``,
    ``score``, ``score0``, ``used`` (B,) int32.  ``max_range``, ``offset``, ``height`` and the sweep are the scan's
    (``LidarPlanes``).  ``set_map(grid, occ_threshold)`` is one launch, ``step(pose, ranges)`` two (project, match) on the
    current (or the given) stream; neither reads the device."""

    def __init__(self, B, H, W, x0, y0, cell, rays, max_range, offset, height, angle_min, angle_max, sub=8, cap=256,
                 nxy=3, step_xy=0.03, nth=4, step_th=0.01, min_hits=8, device=None):
        import torch
        if int(B) < 1 or not 1 <= int(rays) <= _lib.MATCH_MAX_RAYS:
            raise ValueError(f"ScanMatcher: B >= 1 and 1 <= rays <= {_lib.MATCH_MAX_RAYS}")
        if int(H) < 1 or int(W) < 1 or int(H) * int(W) > _lib.GRID_MAX_CELLS:
            raise ValueError(f"ScanMatcher: H, W >= 1 and at most {_lib.GRID_MAX_CELLS} cells")
        if not 1 <= int(sub) <= 8 or not 1 <= int(cap) <= 65535:
            raise ValueError("ScanMatcher: 1 <= sub <= 8 and 1 <= cap <= 65535")
        if not 0 <= int(nxy) <= _lib.MATCH_MAX_N or not 0 <= int(nth) <= _lib.MATCH_MAX_N:
            raise ValueError(f"ScanMatcher: 0 <= nxy, nth <= {_lib.MATCH_MAX_N}")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        i32 = dict(dtype=torch.int32, device=dev)
        self.device = dev
        self.B, self.H, self.W, self.rays = int(B), int(H), int(W), int(rays)
        self.x0, self.y0, self.cell = float(x0), float(y0), float(cell)
        self.max_range, self.offset, self.height = float(max_range), (float(offset[0]), float(offset[1])), float(height)
        self.angle_min, self.angle_max = float(angle_min), float(angle_max)
        self.sub, self.cap, self.min_hits = int(sub), int(cap), int(min_hits)
        self.nxy, self.step_xy, self.nth, self.step_th = int(nxy), float(step_xy), int(nth), float(step_th)
        self.d2 = torch.full((self.H * self.sub, self.W * self.sub), self.cap, **i32)
        self.rot = torch.from_numpy(rotation_table(self.nth, self.step_th)).to(dev)
        self.points = torch.zeros((self.B, self.rays, 3), dtype=torch.float64, device=dev)
        self.pose_out = torch.zeros((self.B, 3), dtype=torch.float64, device=dev)
        self.best, self.score = torch.zeros(self.B, **i32), torch.zeros(self.B, **i32)
        self.score0, self.used = torch.zeros(self.B, **i32), torch.zeros(self.B, **i32)

    def set_map(self, grid, occ_threshold, stream=None):
        """grid (H, W) fp64 on the device: the table ``d2`` of its obstacle faces (cells >= occ_threshold are occupied)"""
        _lib.grid_edge_distance_device(grid, self.d2, occ_threshold, self.sub, self.cap,
                                       stream=_lib.stream_handle(stream, self.device))

    def step(self, pose, ranges, stream=None):
        """pose (B, stride >= 3) the priors, ranges (B, rays) the scan (``LidarPlanes.ranges``).  Returns ``pose_out``
        (B, 3): the lattice pose whose scan end points lie nearest the map's faces, the prior itself for a robot with
        fewer than ``min_hits`` hits (``best`` -1)."""
        st = _lib.stream_handle(stream, self.device)
        _lib.lidar_project_device(pose, ranges, self.points, self.angle_min, self.angle_max, self.max_range, self.offset,
                                  self.height, stream=st)
        a = _lib.scan_match_args(pose, self.points, ranges, self.d2, self.rot, self.pose_out, self.best, self.score,
                                 self.H, self.W, self.sub, self.cap, self.x0, self.y0, self.cell, self.nxy, self.step_xy,
                                 self.nth, self.step_th, self.max_range, self.min_hits, self.score0, self.used)
        _lib.scan_match_device(a, self.B, stream=st)
        return self.pose_out


class ScanSearcher:
    """Wide-window scan matching beside a ``ScanMatcher``: the pose that ``rmpc_scan_match``'s rule picks from a lattice
    of (2 nxy + 1)^2 (2 nth + 1) poses, nxy and nth up to 127, found by branch and bound on the minimum pyramid of the
    matcher's ``d2``.  Shares the matcher's map, lidar, frame and ``min_hits``; owns ``pyr`` (levels, H sub, W sub) int32,
    ``rot``, ``points``, the workspace and ``pose_out`` (B, 3), ``best``, ``score``, ``score0``, ``used``, ``leaves`` (B,)
    int32.  ``levels`` defaults to what the window of a top-level block of 2^top_log2 steps needs.  ``set_map()`` (after
    the matcher's) is one launch per level, ``step`` two (project, search); neither reads the device."""

    def __init__(self, matcher, nxy, step_xy, nth, step_th, top_log2=3, levels=None):
        import math
        import torch
        if not 0 <= int(nxy) <= _lib.SEARCH_MAX_N or not 0 <= int(nth) <= _lib.SEARCH_MAX_N:
            raise ValueError(f"ScanSearcher: 0 <= nxy, nth <= {_lib.SEARCH_MAX_N}")
        if not 0 <= int(top_log2) <= _lib.SEARCH_MAX_TOP:
            raise ValueError(f"ScanSearcher: 0 <= top_log2 <= {_lib.SEARCH_MAX_TOP}")
        m = self.matcher = matcher
        if levels is None:
            levels = min(_lib.SEARCH_MAX_LEVELS,
                         math.ceil(math.log2((1 << int(top_log2)) * float(step_xy) * m.sub / m.cell + 2.0)) + 1)
        if not 1 <= int(levels) <= _lib.SEARCH_MAX_LEVELS:
            raise ValueError(f"ScanSearcher: 1 <= levels <= {_lib.SEARCH_MAX_LEVELS}")
        dev = self.device = m.device
        i32 = dict(dtype=torch.int32, device=dev)
        self.B = m.B
        self.nxy, self.step_xy, self.nth, self.step_th = int(nxy), float(step_xy), int(nth), float(step_th)
        self.top_log2, self.levels = int(top_log2), int(levels)
        self.pyr = torch.full((self.levels, m.H * m.sub, m.W * m.sub), m.cap, **i32)
        self.rot = torch.from_numpy(rotation_table(self.nth, self.step_th)).to(dev)
        self.points = torch.zeros((m.B, m.rays, 3), dtype=torch.float64, device=dev)
        nbytes = 4 * m.B * _lib.scan_search_top_nodes(self.nxy, self.nth, self.top_log2)
        self.work = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.pose_out = torch.zeros((m.B, 3), dtype=torch.float64, device=dev)
        self.best, self.score = torch.zeros(m.B, **i32), torch.zeros(m.B, **i32)
        self.score0, self.used, self.leaves = torch.zeros(m.B, **i32), torch.zeros(m.B, **i32), torch.zeros(m.B, **i32)

    def set_map(self, stream=None):
        """the pyramid of the matcher's ``d2``: call after ``matcher.set_map`` (on the same stream)"""
        _lib.grid_min_pyramid_device(self.matcher.d2, self.pyr, self.matcher.sub,
                                     stream=_lib.stream_handle(stream, self.device))

    def step(self, pose, ranges, active=None, stream=None):
        """pose (B, stride >= 3) the priors, ranges (B, rays) the scan, active (B,) int32 or None: robots with 0 keep
        their prior (``best`` -1).  Returns ``pose_out`` (B, 3), the least pose of the wide lattice by the matcher's rule."""
        m, st = self.matcher, _lib.stream_handle(stream, self.device)
        _lib.lidar_project_device(pose, ranges, self.points, m.angle_min, m.angle_max, m.max_range, m.offset, m.height,
                                  stream=st)
        a = _lib.scan_match_args(pose, self.points, ranges, m.d2, self.rot, self.pose_out, self.best, self.score, m.H, m.W,
                                 m.sub, m.cap, m.x0, m.y0, m.cell, self.nxy, self.step_xy, self.nth, self.step_th,
                                 m.max_range, m.min_hits, self.score0, self.used)
        s = _lib.scan_search_args(a, self.pyr, self.top_log2, self.work, active=active, leaves=self.leaves)
        _lib.scan_search_device(s, self.B, stream=st)
        return self.pose_out

    def relocalize(self, pose, ranges, active=None, stream=None):
        """the search, then the matcher's fine lattice at the search's result: returns the matcher's ``pose_out``.  A
        robot with active 0 is matched at its prior."""
        return self.matcher.step(self.step(pose, ranges, active, stream), ranges, stream)


class OdometryDrift:
    """Wheel odometry of B robots over at most ``steps`` control steps: ``advance`` reads the true signed forward
    displacement ds and heading change dth off two true states, perturbs them to ds (1 + sigma_ds n1) and
    dth + sigma_dth n2 + bias_dth, and integrates them onto the estimate.  ``noise`` (steps, B, 2) is drawn once on the
    host from ``numpy.random.default_rng(seed)``, so that a numpy restatement shares it."""

    def __init__(self, B, steps, seed, sigma_ds=0.05, sigma_dth=0.01, bias_dth=0.002):
        if int(B) < 1 or int(steps) < 1:
            raise ValueError("OdometryDrift: B, steps >= 1")
        self.B, self.steps = int(B), int(steps)
        self.sigma_ds, self.sigma_dth, self.bias_dth = float(sigma_ds), float(sigma_dth), float(bias_dth)
        self.noise = np.random.default_rng(seed).standard_normal((self.steps, self.B, 2))
        self.k = 0                 # the control steps advanced so far
        self._dev = None

    def advance(self, est, x_prev, x_new):
        """est (B, 3) the estimates (x, y, heading), updated in place and returned; x_prev, x_new (B, >= 3) the true
        states before and after the control step.  ds = the displacement along the heading of x_prev."""
        import torch
        if self.k >= self.steps:
            raise ValueError(f"OdometryDrift: the noise table holds {self.steps} steps")
        if self._dev is None or self._dev.device != est.device:
            self._dev = torch.from_numpy(self.noise).to(est.device)
        n = self._dev[self.k]
        self.k += 1
        th = x_prev[:, 2]
        ds = (x_new[:, 0] - x_prev[:, 0]) * torch.cos(th) + (x_new[:, 1] - x_prev[:, 1]) * torch.sin(th)
        ds = ds * (1.0 + self.sigma_ds * n[:, 0])
        dth = (x_new[:, 2] - th) + self.sigma_dth * n[:, 1] + self.bias_dth
        e = est[:, 2].clone()
        est[:, 0] += ds * torch.cos(e)
        est[:, 1] += ds * torch.sin(e)
        est[:, 2] += dth
        return est
