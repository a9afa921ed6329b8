"""``a_star`` with the reference's signature and return format (``robotmpcs/global_planner/a_star.py``), computed on the
device: the cost-to-go field of the goal (``rmpc_grid_fields_device``, on a map of more than ``_lib.GRID_MAX_CELLS``
cells ``rmpc_grid_fields_large_device``) and its descent from the start
(``rmpc_grid_paths_device``).  The path has the least cost delta + occupancy_cost_factor data over its cells, the cost
the reference's A* sums (its doubled potential term in the priority can make that A* return a dearer path on graded
maps; on binary maps both costs agree).  The map's ``visited`` array is left untouched."""
from __future__ import annotations

import numpy as np

from .. import _lib
from .batch import MOVES


def a_star(start_m, goal_m, gmap, movement='8N', occupancy_cost_factor=3):
    import torch
    start = gmap.get_index_from_coordinates(start_m[0], start_m[1])
    goal = gmap.get_index_from_coordinates(goal_m[0], goal_m[1])
    if gmap.is_occupied_idx(start):          # (raises outside the map, as the reference)
        raise Exception('Start node is not traversable')
    if gmap.is_occupied_idx(goal):
        raise Exception('Goal node is not traversable')
    if movement not in ('4N', '8N'):
        raise ValueError('Unknown movement')
    H, W = int(gmap.dim_cells[0]), int(gmap.dim_cells[1])
    dev = torch.device("cuda", 0)
    grid = torch.from_numpy(np.ascontiguousarray(gmap.data, dtype=np.float64)).to(dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    goal_c, start_c = i32([goal[1] * W + goal[0]]), i32([start[1] * W + start[0]])
    fields = torch.empty((1, H, W), dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    path = torch.empty((1, H * W), dtype=torch.int32, device=dev)
    length = torch.empty(1, dtype=torch.int32, device=dev)
    th, f = float(gmap.occupancy_threshold), float(occupancy_cost_factor)
    fields_device = _lib.grid_fields_large_device if H * W > _lib.GRID_MAX_CELLS else _lib.grid_fields_device
    fields_device(grid, goal_c, fields, status, MOVES[movement], th, f)
    _lib.grid_paths_device(grid, fields, goal_c, start_c, i32([0]), path, length, MOVES[movement], th, f)
    n = int(length.item())
    if n < 0:
        raise _lib.RmpcError("rmpc_grid_paths_device: status %d" % n)
    cells = path[0, :n].cpu().numpy()
    path_idx = [(int(c % W), int(c // W)) for c in cells]
    return [gmap.get_coordinates_from_index(x, y) for x, y in path_idx], path_idx
