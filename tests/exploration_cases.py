"""Constructed inputs that the exploration and assignment tests share: seed grids, random evidence, test grids, and the
kinematic exploration of the examples' store driven by the restatements (cached: tests/test_exploration_cpu.py and
tests/test_assignment_cpu.py read the same four runs)."""
import functools
import math

import numpy as np

from exploration_reference import OK, descend_seeded_ref, field_seeded_ref, frontier_ref
from global_planner_reference import inflate_ref
from lidar_reference import scan_ref
from mapping_reference import mark_ref, occupancy_ref
from robot_mpcs_amd.global_planner import FREE, OCC

INF = math.inf


def one_seed(shape, cells, values=None):
    s = np.full(shape, INF)
    s.ravel()[list(cells)] = 0.0 if values is None else values
    return s


def evidence(H, W, kind, rng):
    """(hits, misses, enlarged): "sparse" random evidence on about 40 % of the cells in blobs and single cells"""
    if kind == "unknown":
        hits = misses = np.zeros((H, W), dtype=np.int32)
    elif kind == "known":
        hits, misses = rng.integers(0, 3, (H, W)).astype(np.int32), rng.integers(1, 9, (H, W)).astype(np.int32)
    else:
        known = rng.uniform(size=(H, W)) < 0.15
        for _ in range(max(1, H * W // 200)):
            r, c, h, w = rng.integers(0, H), rng.integers(0, W), rng.integers(1, 12), rng.integers(1, 12)
            known[r:r + h, c:c + w] = True
        hits = np.where(known & (rng.uniform(size=(H, W)) < 0.3), rng.integers(1, 5, (H, W)), 0).astype(np.int32)
        misses = np.where(known & (hits == 0), rng.integers(1, 50, (H, W)), 0).astype(np.int32)
        hits[0, 0], misses[0, 0] = -(1 << 31), -(1 << 31)     # wrapped counters: known in 64 bits, 0 in 32
    enlarged = (rng.uniform(size=(H, W)) < 0.3).astype(np.float64)
    return hits, misses, enlarged


def grid_of(H, W, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "store":
        from robot_mpcs_amd.global_planner import shelf_map
        big = H >= 100
        return shelf_map(H, W, seed=3, aisle=9 if big else 6, shelf=4 if big else 2, gap=6 if big else 5)
    occ = rng.uniform(size=(H, W)) < 0.25
    if kind == "binary":
        return occ.astype(np.float64)
    return np.where(occ, 1.0, rng.uniform(0.0, 0.7, (H, W)))


def explore_kinematic(seed, B, max_steps=1500, replan_every=5, rays=64, max_range=10.0):
    """Robots without a map or goals in the examples' store (robot_mpcs_amd/store.py), packed into one corner, in the order of
    that example's control step (follower -> scan -> mark -> re-plan -> move): the follower moves on by one waypoint;
    the robot scans from its cell's centre and the scan is marked; every replan_every steps the evidence is classified
    with unknown = free, enlarged, the frontier found, the seeded field built and one descent per robot made, which
    restarts the route at the robot's own cell (RouteFollower.replace); then the robot stands on its waypoint.  So a
    re-plan step moves nobody, and a route is followed for replan_every - 1 cells before the next one.  Returns the step
    of the first re-plan without a frontier (None if there was none), the free cells and those among them never seen,
    and the number of robot-steps spent on a cell of the truly enlarged map."""
    from robot_mpcs_amd.global_planner import png_values
    from robot_mpcs_amd.store import STORE, store_map
    from robot_mpcs_amd.utils.exploration import corner_starts
    from robot_mpcs_amd.utils.lidar import boxes_from_grid
    H, W, cell, x0 = STORE.H, STORE.W, STORE.cell, STORE.x0
    raw = store_map(seed)
    boxes = boxes_from_grid(raw, x0, x0, cell)
    truly_enlarged = inflate_ref(png_values(raw), cell, STORE.size_robot, 0.29)[0] > 0.5
    cells = corner_starts(raw, B).astype(np.int64)
    hits, misses = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    routes, idx = [[int(c)] for c in cells], [0] * B
    ended, on_enlarged = None, 0
    for step in range(max_steps):
        for b in range(B):
            if idx[b] < len(routes[b]) - 1:
                idx[b] += 1
        pose = np.stack([x0 + (cells % W) * cell, x0 + (cells // W) * cell, np.zeros(B)], 1)
        pts, t, _ = scan_ref(pose, rays, -math.pi, math.pi, max_range, (0.0, 0.0), 0.02, boxes)
        org = np.concatenate([pose[:, :2], np.full((B, 1), 0.02)], 1)
        _, _, skipped = mark_ref(org, pts, t, H, W, x0, x0, cell, max_range, 1e-6, hits, misses)
        assert skipped == 0
        if step % replan_every == 0:
            grid, _, _ = occupancy_ref(hits, misses, 3, 1, 0, FREE, OCC, FREE)
            enlarged, _ = inflate_ref(grid, cell, STORE.size_robot, 0.29)
            plan, seeds, count = frontier_ref(hits, misses, enlarged)
            if count == 0:
                ended = step
                break
            D, status = field_seeded_ref(plan, seeds)
            assert status == OK
            for b in range(B):
                path, n = descend_seeded_ref(plan, D, seeds, int(cells[b]), max_len=4 * (H + W))
                if n > 0:
                    routes[b], idx[b] = path, 0
        for b in range(B):
            cells[b] = routes[b][idx[b]]
        on_enlarged += int(truly_enlarged.ravel()[cells].sum())
    free = raw < 0.5
    unseen = free & (hits + misses == 0)
    return dict(ended=ended, free=int(free.sum()), unseen=int(unseen.sum()), on_enlarged=on_enlarged)


KINEMATIC = [(0, 1, 1371), (0, 8, 1371), (0, 32, 1371), (3, 8, 1365)]     # (store seed, robots, free cells of the store)


@functools.lru_cache(maxsize=None)
def kinematic(seed, B):
    r = explore_kinematic(seed, B)
    print(dict(seed=seed, B=B, **r))
    return r
