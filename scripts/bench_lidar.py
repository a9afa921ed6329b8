#!/usr/bin/env python3
"""Throughput of the lidar chain on one GPU: the scan (rmpc_lidar_scan_device), the per-stage seeds
(rmpc_plan_points_device) and the free-space decomposition (rmpc_free_space_device), R = 64 rays, N = 10 stages,
B = 256 and 4096 robots, K = 1 and 4 planes, in two worlds: the examples' store (robot_mpcs_amd/store.py: 41 x 41
cells of 0.45 m) and a 128 x 128 store (0.15 m cells), both merged into boxes by boxes_from_grid.

  - times are medians of --reps event-timed launches (each synchronised), after one warm-up launch;
  - rays/s and box tests/s of the scan (B R and B R nbox over its time);
  - the per-robot numpy restatement of tests/lidar_reference.py (scan_ref, plan_points_ref, oracle/fsd_numpy.py) on the
    host CPU of the same box, one robot at a time: a yardstick of the scale, not a tuned CPU baseline.

    timeout -k 10 300 python scripts/bench_lidar.py [--reps 20]

Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def cpu_ms_per_robot(pose, boxes, N, K, robots=8):
    """Median ms of the numpy restatement for one robot: scan, seeds, N decompositions."""
    from oracle.fsd_numpy import free_space_decomposition
    from lidar_reference import plan_points_ref, scan_ref
    times = []
    for b in range(robots):
        t0 = time.perf_counter()
        pts, _, _ = scan_ref(pose[b:b + 1], 64, -math.pi, math.pi, 10.0, (0.4, 0.0), 0.02, boxes)
        seeds = plan_points_ref(pose[b:b + 1], N)
        for k in range(N):
            free_space_decomposition(pts[0], seeds[0, k], K, 5.0)
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import event_ms
    from robot_mpcs_amd.global_planner import shelf_map
    from robot_mpcs_amd.store import STORE
    from robot_mpcs_amd.utils.lidar import boxes_from_grid

    dev = "cuda:0"
    rng = np.random.default_rng(0)
    R, N = 64, 10
    res = {}
    for H, cell, kw in ((STORE.H, STORE.cell, dict(aisle=STORE.aisle, shelf=STORE.shelf, gap=STORE.gap)),
                        (128, 0.15, dict(aisle=9, shelf=4, gap=6))):
        raw = shelf_map(H, H, seed=0, **kw)
        x0 = -0.5 * (H - 1) * cell
        boxes_np = boxes_from_grid(raw, x0, x0, cell)
        boxes = torch.from_numpy(boxes_np).to(dev)
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
            pts = torch.empty((B, R, 3), dtype=torch.float64, device=dev)
            seeds = torch.empty((B, N, 3), dtype=torch.float64, device=dev)
            scan_ms = event_ms(lambda: _lib.lidar_scan_device(pose, pts, boxes), a.reps)
            plan_ms = event_ms(lambda: _lib.plan_points_device(pose, seeds, z, ef), a.reps)
            r[f"B{B}_scan_ms"] = round(scan_ms, 4)
            r[f"B{B}_rays_per_s"] = round(1e3 * B * R / scan_ms)
            r[f"B{B}_box_tests_per_s"] = round(1e3 * B * R * len(boxes_np) / scan_ms)
            r[f"B{B}_plan_points_ms"] = round(plan_ms, 4)
            for K in (1, 4):
                planes = torch.empty((B, N, K, 4), dtype=torch.float64, device=dev)
                fsd_ms = event_ms(lambda: _lib.free_space_decomposition_device(pts, seeds, planes, 5.0), a.reps)
                r[f"B{B}_K{K}_fsd_ms"] = round(fsd_ms, 4)
                r[f"B{B}_K{K}_chain_ms"] = round(scan_ms + plan_ms + fsd_ms, 4)
        for K in (1, 4):
            r[f"cpu_numpy_K{K}_ms_per_robot"] = round(cpu_ms_per_robot(pose_np, boxes_np, N, K), 3)
        res[f"{H}x{H}"] = r
    print(json.dumps(dict(bench="lidar", device=torch.cuda.get_device_name(0), rays=R, N=N, results=res)))


if __name__ == "__main__":
    main()
