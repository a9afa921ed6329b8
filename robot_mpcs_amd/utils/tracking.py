"""What moves around a robot: ``ObstacleTracker`` turns each robot's own lidar scan into the ``obst_dyn`` array a scene
points at -- the returns that the known static world does not explain, their segments, one circle of
known radius per segment, an alpha-beta filter per track (``rmpc_lidar_tracks_device``).  The loops before it copied the
simulator's truth into ``obst_dyn``; a robot on a shop floor has its scan.  There is no CPU path.
"""
from __future__ import annotations

import math

import numpy as np

from .. import _lib


class ObstacleTracker:
    """Scan -> moving returns -> circle detections -> tracks -> ``obst_dyn`` for B robots.

    Owns the buffers: ``points`` (B, rays, 3), ``ranges`` and ``static_ranges`` (B, rays), ``origin`` (B, 3), the
    filter's state ``track`` (B, n_tracks, 4) = (px, py, vx, vy), ``age`` and ``miss`` (B, n_tracks) int32, the
    outputs ``obst_dyn`` (B, n_out, 9), ``det`` (B, 16, 2) and ``counts`` (B, 4) int32 (segments, detections, live and
    confirmed tracks).  ``boxes`` (nbox, 4) is the known static world (``boxes_from_grid`` of the map): a return counts
    as moving when it is ``margin`` shorter than the scan of the boxes alone, without boxes when it is shorter than
    ``max_range``.  ``step`` and ``step_ranges`` enqueue their launches on the current (or the given) stream and never
    synchronise.  The sensor's defaults are the boxer's (``LidarPlanes``); ``radius`` is the one radius all moving
    obstacles are taken to have, which is also the scene's ``dyn_radius`` (``make_block(..., dyn_radius=radius)``)."""

    def __init__(self, B, n_out, boxes=None, rays=256, n_tracks=8, radius=0.3, dt=0.1, angle_min=-math.pi,
                 angle_max=math.pi, max_range=10.0, offset=(0.4, 0.0), height=0.02, margin=0.05, gap=None, min_rays=2,
                 max_extent=None, gate=1.0, alpha=0.4, beta=0.1, v_max=0.0, confirm=3, max_miss=5, park=(100.0, 100.0),
                 device=None):
        import torch
        if int(B) < 1 or int(n_out) < 1:
            raise ValueError("ObstacleTracker: B, n_out >= 1")
        if not 1 <= int(rays) <= _lib.TRACK_MAX_RAYS or not 1 <= int(n_tracks) <= _lib.TRACK_MAX_TRACKS:
            raise ValueError(f"ObstacleTracker: 1 <= rays <= {_lib.TRACK_MAX_RAYS} and 1 <= n_tracks <= "
                             f"{_lib.TRACK_MAX_TRACKS}")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
        self.device = dev
        self.B, self.n_out, self.rays, self.n_tracks = int(B), int(n_out), int(rays), int(n_tracks)
        self.boxes = torch.as_tensor(np.zeros((0, 4)) if boxes is None else boxes, dtype=torch.float64).reshape(-1, 4) \
            .to(dev).contiguous()
        self.angle_min, self.angle_max, self.max_range = float(angle_min), float(angle_max), float(max_range)
        self.offset, self.height = (float(offset[0]), float(offset[1])), float(height)
        self.radius, self.dt = float(radius), float(dt)
        # a full sweep closes on itself; neighbouring returns on one obstacle lie within 1.5 radii of each other as long
        # as three rays hit it (the widest step is the one onto the rim)
        self.closed = abs((self.angle_max - self.angle_min) - 2.0 * math.pi) <= 1e-12
        self.gap = 1.5 * float(radius) if gap is None else float(gap)
        self.max_extent = 2.0 * float(radius) + 0.1 if max_extent is None else float(max_extent)
        self.points = torch.zeros((self.B, self.rays, 3), **f64)
        self.ranges = torch.zeros((self.B, self.rays), **f64)
        self.static_ranges = torch.zeros((self.B, self.rays), **f64) if self.boxes.shape[0] else None
        self._static_points = torch.zeros((self.B, self.rays, 3), **f64) if self.boxes.shape[0] else None
        self.origin = torch.zeros((self.B, 1, 3), **f64)
        self.track = torch.zeros((self.B, self.n_tracks, 4), **f64)
        self.age, self.miss = torch.zeros((self.B, self.n_tracks), **i32), torch.zeros((self.B, self.n_tracks), **i32)
        self.obst_dyn = torch.zeros((self.B, self.n_out, 9), **f64)
        self.obst_dyn[:, :, 0], self.obst_dyn[:, :, 1] = float(park[0]), float(park[1])
        self.det = torch.zeros((self.B, _lib.TRACK_MAX_DET, 2), **f64)
        self.counts = torch.zeros((self.B, 4), **i32)
        self.args = _lib.tracks_args(self.points, self.ranges, self.origin, self.track, self.age, self.miss, self.obst_dyn,
                                     self.radius, self.dt, static_ranges=self.static_ranges, closed=self.closed,
                                     max_range=self.max_range, margin=margin, gap=self.gap, min_rays=min_rays,
                                     max_extent=self.max_extent, gate=gate, alpha=alpha, beta=beta, v_max=v_max,
                                     confirm=confirm, max_miss=max_miss, park=park, det=self.det, counts=self.counts)

    def reset(self):
        """forget every track (the state's zero fill); ``obst_dyn`` keeps its rows until the next step"""
        self.track.zero_(); self.age.zero_(); self.miss.zero_()

    def _track(self, pose, st):
        if self.static_ranges is not None:
            _lib.lidar_scan_device(pose, self._static_points, self.boxes, None, self.angle_min, self.angle_max,
                                   self.max_range, self.offset, self.height, ranges=self.static_ranges, stream=st)
        _lib.plan_points_device(pose, self.origin, None, None, self.offset, self.height, stream=st)
        _lib.lidar_tracks_device(self.args, self.B, stream=st)
        return self.obst_dyn

    def step(self, xinit, circles, stream=None, bodies=None):
        """xinit (B, stride >= 3) the poses, circles (P, 3) = (cx, cy, r) what moves in the world now or None, bodies
        (centres, radius, self0) the fleet's robots as ``LidarPlanes.step`` takes them or None (device tensors).
        Scans the boxes and the circles (with bodies: and the other robots, ``rmpc_lidar_scan_fleet_device``), scans the
        boxes alone (skipped without boxes), takes the sensor origins and runs the tracker.  Returns ``obst_dyn``."""
        st = _lib.stream_handle(stream, self.device)
        self.args.ranges = self.ranges.data_ptr()
        if bodies is None:
            _lib.lidar_scan_device(xinit, self.points, self.boxes, circles, self.angle_min, self.angle_max,
                                   self.max_range, self.offset, self.height, ranges=self.ranges, stream=st)
        else:
            centres, radius, self0 = bodies
            _lib.lidar_scan_fleet_device(xinit, self.points, centres, radius, self.boxes, circles, self.angle_min,
                                         self.angle_max, self.max_range, self.offset, self.height, self0=self0,
                                         ranges=self.ranges, stream=st)
        return self._track(xinit, st)

    def step_ranges(self, pose, ranges, stream=None):
        """pose (B, stride >= 3) the believed poses, ranges (B, rays) the measured scan: the points are the ranges
        placed at that pose (``rmpc_lidar_project_device``), the static world is scanned from it.  Returns
        ``obst_dyn``."""
        st = _lib.stream_handle(stream, self.device)
        self.args.ranges, self._measured = ranges.data_ptr(), ranges            # read in place: no copy, no torch op
        _lib.lidar_project_device(pose, ranges, self.points, self.angle_min, self.angle_max, self.max_range,
                                  self.offset, self.height, stream=st)
        return self._track(pose, st)
