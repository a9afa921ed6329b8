#!/usr/bin/env python3
"""Time of the mapping kernels on one GPU beside the lidar chain that feeds them: ``FleetMap.mark`` (the origins
launch and k_grid_mark: one lane per ray, global atomics) and k_grid_occupancy, against ``LidarPlanes.step`` (scan,
seeds, free-space decomposition; N = 10, K = 4) at the same B.  The worlds and sizes of scripts/bench_lidar.py: the
examples' store (robot_mpcs_amd/store.py: 41 x 41 cells of 0.45 m) and a 128 x 128 store (0.15 m cells), R = 64 rays of
range 10, B = 256 and 4096 robots on free cells.

  - times are medians of --reps event-timed launches (each synchronised), after one warm-up launch;
  - visits: the cell updates of one scan (the sum of both grids after one call), unique: the map cells it touches.

    timeout -k 10 300 python scripts/bench_mapping.py [--reps 20]

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
    from robot_mpcs_amd.fleet import event_ms
    from robot_mpcs_amd.global_planner import FREE, OCC, shelf_map
    from robot_mpcs_amd.store import STORE
    from robot_mpcs_amd.utils.lidar import LidarPlanes, boxes_from_grid
    from robot_mpcs_amd.utils.mapping import FleetMap

    dev = "cuda:0"
    rng = np.random.default_rng(0)
    R, N, K = 64, 10, 4
    res = {}
    for H, cell, max_range, kw in ((STORE.H, STORE.cell, 10.0, dict(aisle=STORE.aisle, shelf=STORE.shelf, gap=STORE.gap)),
                                   (128, 0.15, 10.0, dict(aisle=9, shelf=4, gap=6))):
        raw = shelf_map(H, H, seed=0, **kw)
        x0 = -0.5 * (H - 1) * cell
        boxes_np = boxes_from_grid(raw, x0, x0, cell)
        free = np.flatnonzero(raw.ravel() < 0.5)
        r = dict(nbox=int(len(boxes_np)))
        for B in (256, 4096):
            c = rng.choice(free, B)
            pose_np = np.zeros((B, 8))
            pose_np[:, 0], pose_np[:, 1] = x0 + (c % H) * cell, x0 + (c // H) * cell
            pose_np[:, 2] = rng.uniform(-math.pi, math.pi, B)
            pose = torch.from_numpy(pose_np).to(dev)
            z = pose[:, None, :].repeat(1, N, 1).contiguous()
            ef = torch.zeros(B, dtype=torch.int32, device=dev)
            lp = LidarPlanes(B, N, K, boxes=boxes_np, rays=R, max_range=max_range, device=dev)
            fmap = FleetMap(B, H, H, x0, x0, cell, R, max_range, lp.offset, lp.height, device=dev)
            r[f"B{B}_lidar_step_ms"] = round(event_ms(lambda: lp.step(pose, z, ef), a.reps), 4)
            fmap.mark(pose, lp.points, lp.ranges)
            torch.cuda.synchronize()
            h, m = fmap.hits.clone(), fmap.misses.clone()
            r[f"B{B}_mark_ms"] = round(event_ms(lambda: fmap.mark(pose, lp.points, lp.ranges), a.reps), 4)
            r[f"B{B}_visits"] = int(h.sum().item() + m.sum().item())
            r[f"B{B}_unique_cells"] = int(((h + m) > 0).sum().item())
            r[f"B{B}_occupancy_ms"] = round(event_ms(lambda: fmap.occupancy(FREE, OCC, FREE), a.reps), 4)
        res[f"{H}x{H}"] = r
    print(json.dumps(dict(bench="mapping", device=torch.cuda.get_device_name(0), rays=R, N=N, K=K, results=res)))


if __name__ == "__main__":
    main()
