"""``GlobalPlanner`` with the reference's constructor and methods (``robotmpcs/global_planner/globalPlanner.py``).

The single-robot coordinate arithmetic (``convert_meters``, ``convert_meters_reversed``, ``get_local_goal``) runs on the
host in the reference's operation order; enlarging the obstacles and the path search run on the device.

Deviations: plotting is left out (``BOOL_PLOTTING`` is accepted and ignored).  The reference writes its 2-D occupancy
map to ``occupancy_map.png`` with ``plt.imsave`` and reads it back with ``OccupancyGridMap.from_png``; here no file is
written: ``get_occupancy_map`` computes the values that round trip yields (``png_values``: min-max scaling, the viridis
colour map, first plane / 256, rows reversed) directly, and ``set_occupancy_map`` takes a map already in the planner's
image frame.  The values matter: free cells read 68/256 and occupied ones 253/256, so the blur-and-threshold of
``get_enlarged_obstacles`` (mean > 0.29) blocks every cell within k of an obstacle -- a full dilation.
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from .a_star import a_star
from .gridmap import OccupancyGridMap


def png_values(map2d):
    """What ``from_png`` reads back from ``plt.imsave(path, map2d)``: the map min-max scaled to [0, 1] (a constant map to
    0), through matplotlib's default colour map (viridis, 8 bits per channel), first plane / 256; rows as in ``map2d``
    (``from_png`` reverses them).  For a map of two values: 68/256 on the lower one, 253/256 on the upper one."""
    from matplotlib import colormaps
    m = np.asarray(map2d, dtype=np.float64)
    lo, hi = float(m.min()), float(m.max())
    scaled = (m - lo) / (hi - lo) if hi > lo else np.zeros_like(m)
    return colormaps["viridis"](scaled, bytes=True)[..., 0].astype(np.float64) / 256.0


FREE, OCC = 68.0 / 256.0, 253.0 / 256.0    # png_values of a map of two values: what grid_inflate_device gets in the reference


class GlobalPlanner(object):
    def __init__(self, dim_pixels, limits_low, limits_high, BOOL_PLOTTING=True, threshold=0.29,
                 convolution_blur=(5, 5), enlarge_obstacles=True, threshold_local_goal=1.3):
        self.dim_pixels = dim_pixels
        self.limits_high = limits_high
        self.limits_low = limits_low
        self.dim_meters = -limits_low + limits_high
        self.cell_size_xyz = self.dim_meters / dim_pixels
        self.threshold = threshold
        self.enlarge_obstacles = enlarge_obstacles
        self.convolution_blur = convolution_blur
        self.idx_local = 0
        self.threshold_local_goal = threshold_local_goal
        if self.cell_size_xyz[0] != self.cell_size_xyz[1]:
            print("The voxels must have the same size [meter x meter] in the x, y direction! Please correct!!")
        self.cell_size = self.cell_size_xyz[0]
        self.BOOL_PLOTTING = BOOL_PLOTTING
        self.occupancy_map = None

    def get_occupancy_map(self, sensor, occupancy_map_3D):
        self.occupancy_map_2D = np.clip(np.sum(occupancy_map_3D, axis=2), 0, self.threshold)
        self.set_occupancy_map(png_values(self.occupancy_map_2D)[::-1])
        return sensor

    def set_occupancy_map(self, data):
        """The occupancy map (rows, cols) in the image frame of ``convert_meters``, values in [0, 1]."""
        self.occupancy_map = np.ascontiguousarray(data, dtype=np.float64)

    def get_enlarged_obstacles(self, size_robot=0.4):
        import torch
        if self.occupancy_map is None:
            raise ValueError("no occupancy map: call get_occupancy_map or set_occupancy_map first")
        size_robot_pixels = int(np.ceil(size_robot / self.cell_size))
        self.kernel = np.ones((size_robot_pixels * 2 + 1, size_robot_pixels * 2 + 1))
        dev = torch.device("cuda", 0)
        grid = torch.from_numpy(self.occupancy_map).to(dev)
        out = torch.empty_like(grid)
        _lib.grid_inflate_device(grid, out, float(self.cell_size), float(size_robot), float(self.threshold))
        self.occupancy_map_enlarged = out.cpu().numpy()
        return self.occupancy_map_enlarged

    def convert_meters(self, pos_meters):
        pos_meters_update = pos_meters - self.limits_low
        return [pos_meters_update[1], self.dim_meters[1] - pos_meters_update[0], pos_meters[2]]

    def convert_meters_reversed(self, pos_meters):
        if len(pos_meters) == 2:
            pos_meters = tuple(pos_meters) + (0.0,)
        pos_meters_update = [self.dim_meters[1] - pos_meters[1], pos_meters[0], pos_meters[2]]
        return pos_meters_update + self.limits_low

    def convert_path(self, path):
        return [self.convert_meters_reversed(position) for position in path]

    def get_global_path_astar(self, start_pos, goal_pos):
        if self.occupancy_map is None:
            raise ValueError("no occupancy map: call get_occupancy_map or set_occupancy_map first")
        gmap = OccupancyGridMap(self.occupancy_map.copy(), cell_size=self.cell_size)
        if self.enlarge_obstacles:
            gmap.data = self.get_enlarged_obstacles()
        start_pos = self.convert_meters(np.asarray(start_pos, dtype=np.float64))
        goal_pos = self.convert_meters(np.asarray(goal_pos, dtype=np.float64))
        path, path_px = a_star(start_pos, goal_pos, gmap, movement='8N')
        print("path is feasible" if path else 'Goal is not reachable')
        return self.convert_path(path), path_px

    def get_distance_points(self, position1, position2):
        return np.sqrt((position2[0] - position1[0]) ** 2 + (position2[1] - position1[1]) ** 2)

    def get_local_goal(self, position, path):
        distance_pos_path = self.get_distance_points(position, path[self.idx_local])
        if self.idx_local < len(path) - 1 and len(path) > 0:
            if distance_pos_path <= self.threshold_local_goal:
                self.idx_local = self.idx_local + 1
        return path[self.idx_local]
