"""Constructed inputs that the localisation tests share (tests/test_localization_cpu.py, tests/test_gpu_localization.py):
the store's lidar, its true map with the edge-distance table (cached, read only), and poses clear of the shelves."""
import functools
import math

import numpy as np

from localization_reference import edge_distance_ref
from robot_mpcs_amd.store import STORE, clear_cells, store_map
from robot_mpcs_amd.utils.lidar import boxes_from_grid

LIDAR = dict(rays=64, angle_min=-math.pi, angle_max=math.pi, max_range=10.0, offset=(STORE.ee_offset, 0.0), height=0.02)


@functools.lru_cache(maxsize=None)
def store_world(seed=0, sub=8, cap=256):
    """(raw, boxes, d2) of the store: the true map, the boxes the lidar sees, the edge-distance table; read only"""
    raw = store_map(seed)
    d2 = edge_distance_ref(raw, 0.5, sub, cap)
    d2.setflags(write=False)
    return raw, boxes_from_grid(raw, STORE.x0, STORE.y0, STORE.cell), d2


def clear_poses(raw, n, rng, k, jitter):
    """n poses on cells with no shelf within k cells, moved by up to `jitter` m in x and y, any heading"""
    cells = np.flatnonzero(clear_cells(raw, k).ravel())
    pick = rng.choice(cells, n, replace=len(cells) < n)
    pose = np.zeros((n, 3))
    pose[:, 0] = STORE.x0 + (pick % STORE.W) * STORE.cell + rng.uniform(-jitter, jitter, n)
    pose[:, 1] = STORE.y0 + (pick // STORE.W) * STORE.cell + rng.uniform(-jitter, jitter, n)
    pose[:, 2] = rng.uniform(-math.pi, math.pi, n)
    return pose
