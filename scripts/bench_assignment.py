#!/usr/bin/env python3
"""Time of coordinated exploration on one GPU: each of the three entries alone and the whole re-plan.

  - ``grid_targets_device`` (with tseeds), ``grid_route_costs_device`` and ``assign_greedy_device`` at
    (B, T) = (64, 36), (256, 36) and (4096, 256): T = 36 is the examples' store (41 x 41 cells) in tiles of 8, T = 256 a
    128 x 128 store in tiles of 8.  A twentieth of the free cells are sources, the robots stand on random cells (shelf
    cells included), the fields are those of the targets.  The assignment is timed on that cost matrix (B routes to at
    most T targets, many of them +inf) and on a matrix of uniform doubles of the same shape, with its passes;
  - ``FrontierGoals.replan`` with tile = 8 and with tile = 0 (every robot to the nearest frontier cell) at B = 64 and
    256 robots in a corner of the examples' store, after one marked scan.

Times are medians of --reps event-timed calls (each synchronised), after one warm-up call.

    timeout -k 10 300 python scripts/bench_assignment.py [--reps 20]

Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import event_ms
    from robot_mpcs_amd.global_planner import RouteFollower, shelf_map
    from robot_mpcs_amd.store import STORE
    from robot_mpcs_amd.utils.exploration import FrontierGoals, corner_starts
    from robot_mpcs_amd.utils.lidar import LidarPlanes, boxes_from_grid
    from robot_mpcs_amd.utils.mapping import FleetMap

    dev = "cuda:0"
    rng = np.random.default_rng(0)
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    inf = float("inf")
    store = dict(aisle=STORE.aisle, shelf=STORE.shelf, gap=STORE.gap)
    entries = {}
    for B, H, kw in ((64, STORE.H, store), (256, STORE.H, store), (4096, 128, dict(aisle=9, shelf=4, gap=6))):
        raw = shelf_map(H, H, seed=0, **kw)
        free = np.flatnonzero(raw.ravel() < 0.5)
        seed_np = np.full(H * H, inf)
        seed_np[rng.choice(free, len(free) // 20, replace=False)] = 0.0
        grid = torch.from_numpy(raw.astype(np.float64)).to(dev)
        seed = torch.from_numpy(seed_np.reshape(H, H)).to(dev)
        T = _lib.grid_tiles(H, H, 8)
        targets, tseeds = torch.zeros(T, **i32), torch.zeros((T, H, H), **f64)
        fields, status = torch.zeros((T, H, H), **f64), torch.zeros(T, **i32)
        cells = torch.from_numpy(rng.integers(0, H * H, B).astype(np.int32)).to(dev)
        cost, assign, passes = torch.zeros((B, T), **f64), torch.zeros(B, **i32), torch.zeros(B, **i32)
        r = dict(map=f"{H}x{H}")
        r["targets_ms"] = round(event_ms(lambda: _lib.grid_targets_device(seed, 8, targets, tseeds), a.reps), 4)
        _lib.grid_fields_seeded_device(grid, tseeds, fields, status)
        r["fields_ms"] = round(event_ms(lambda: _lib.grid_fields_seeded_device(grid, tseeds, fields, status), a.reps), 4)
        r["route_costs_ms"] = round(event_ms(lambda: _lib.grid_route_costs_device(grid, fields, cells, cost), a.reps), 4)
        r["assign_route_ms"] = round(event_ms(lambda: _lib.assign_greedy_device(cost, assign, passes), a.reps), 4)
        r["targets_found"] = int((targets >= 0).sum().item())
        r["assign_route_passes"] = int(passes.max().item()) + 1
        r["assign_route_unassigned"] = int((assign < 0).sum().item())
        uniform = torch.from_numpy(rng.uniform(0.0, 100.0, (B, T))).to(dev)
        r["assign_uniform_ms"] = round(event_ms(lambda: _lib.assign_greedy_device(uniform, assign, passes), a.reps), 4)
        r["assign_uniform_passes"] = int(passes.max().item()) + 1
        entries[f"B{B}_T{T}"] = r

    replan = {}
    H = W = STORE.H
    cell, x0 = STORE.cell, STORE.x0
    raw = shelf_map(H, W, seed=0, **store)
    for B in (64, 256):
        starts = corner_starts(raw, B)
        pose = np.zeros((B, 8))
        pose[:, 0], pose[:, 1] = x0 + (starts % W) * cell, x0 + (starts // W) * cell
        pose[:, 2] = rng.uniform(-math.pi, math.pi, B)
        tx = torch.from_numpy(pose).to(dev)
        lp = LidarPlanes(B, 3, 2, boxes=boxes_from_grid(raw, x0, x0, cell), device=dev)
        fmap = FleetMap(B, H, W, x0, x0, cell, 64, lp.max_range, lp.offset, lp.height, device=dev)
        lp.step(tx)
        fmap.mark(tx, lp.points, lp.ranges)
        r = {}
        for tile in (0, 8):
            fg = FrontierGoals(fmap, STORE.size_robot, 0.29, tile=tile)
            fol = RouteFollower(torch.zeros((B, fg.max_len), **i32), torch.ones(B, **i32), W, x0, x0, cell)
            r[f"tile{tile}_replan_ms"] = round(event_ms(lambda: fg.replan(fol, tx), a.reps), 4)
            r[f"tile{tile}_frontier_cells"] = fg.frontier_cells()
            if tile:
                r["targets_found"] = int((fg.targets >= 0).sum().item())
                r["passes"] = int(fg.passes.max().item()) + 1
                r["field_sweeps_max"] = int(fg.sweeps.max().item())
        replan[f"B{B}"] = r
    print(json.dumps(dict(bench="assignment", device=torch.cuda.get_device_name(0), reps=a.reps, entries=entries,
                          replan=replan)))


if __name__ == "__main__":
    main()
