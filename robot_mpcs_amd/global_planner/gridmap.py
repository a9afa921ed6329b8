"""``OccupancyGridMap`` with the reference's method names and cell conventions (``robotmpcs/global_planner/gridmap.py``).

A point index is ``(x_index, y_index)`` = (column, row) of ``data[row][col]``; a cell's centre lies at
``(x_index * cell_size, y_index * cell_size)`` and a point maps to ``round(x / cell_size)`` (Python's round: half to
even).  The bounds test compares the column with the number of columns and the row with the number of rows (the
reference compares both with ``dim_cells[0]``, the same thing on its square maps).  Plotting is left out.
"""
from __future__ import annotations

import numpy as np


class OccupancyGridMap:
    def __init__(self, data_array, cell_size, occupancy_threshold=0.8):
        self.data = data_array
        self.dim_cells = data_array.shape
        self.dim_meters = (self.dim_cells[0] * cell_size, self.dim_cells[1] * cell_size)
        self.cell_size = cell_size
        self.occupancy_threshold = occupancy_threshold
        self.visited = np.zeros(self.dim_cells, dtype=np.float32)

    def _check(self, point_idx):
        if not self.is_inside_idx(point_idx):
            raise Exception('Point is outside map boundary')
        return point_idx

    def mark_visited_idx(self, point_idx):
        x_index, y_index = self._check(point_idx)
        self.visited[y_index][x_index] = 1.0

    def mark_visited(self, point):
        return self.mark_visited_idx(self.get_index_from_coordinates(point[0], point[1]))

    def is_visited_idx(self, point_idx):
        x_index, y_index = self._check(point_idx)
        return bool(self.visited[y_index][x_index] == 1.0)

    def is_visited(self, point):
        return self.is_visited_idx(self.get_index_from_coordinates(point[0], point[1]))

    def get_data_idx(self, point_idx):
        x_index, y_index = self._check(point_idx)
        return self.data[y_index][x_index]

    def get_data(self, point):
        return self.get_data_idx(self.get_index_from_coordinates(point[0], point[1]))

    def set_data_idx(self, point_idx, new_value):
        x_index, y_index = self._check(point_idx)
        self.data[y_index][x_index] = new_value

    def set_data(self, point, new_value):
        self.set_data_idx(self.get_index_from_coordinates(point[0], point[1]), new_value)

    def is_inside_idx(self, point_idx):
        x_index, y_index = point_idx
        return 0 <= x_index < self.dim_cells[1] and 0 <= y_index < self.dim_cells[0]

    def is_inside(self, point):
        return self.is_inside_idx(self.get_index_from_coordinates(point[0], point[1]))

    def is_occupied_idx(self, point_idx):
        return bool(self.get_data_idx(point_idx) >= self.occupancy_threshold)

    def is_occupied(self, point):
        return self.is_occupied_idx(self.get_index_from_coordinates(point[0], point[1]))

    def get_index_from_coordinates(self, x, y):
        return int(round(x / self.cell_size)), int(round(y / self.cell_size))

    def get_coordinates_from_index(self, x_index, y_index):
        return x_index * self.cell_size, y_index * self.cell_size

    @staticmethod
    def from_png(filename, cell_size):
        """First plane of the image / 2**bitdepth, bottom image row first (origin 'lower'); read with pypng when it is
        installed, with Pillow otherwise."""
        try:
            import png
        except ImportError:
            png = None
        if png is not None:
            width, height, rows, info = png.Reader(filename).read()
            planes, depth = info["planes"], info["bitdepth"]
            arr = np.array([np.asarray(r)[::planes] for r in rows], dtype=np.float64)
        else:
            from PIL import Image
            img = Image.open(filename)
            depth = {"1": 1, "I;16": 16, "I;16B": 16, "I": 32}.get(img.mode, 8)
            a = np.asarray(img)
            arr = (a[..., 0] if a.ndim == 3 else a).astype(np.float64)
        return OccupancyGridMap(arr[::-1] / 2 ** depth, cell_size)
