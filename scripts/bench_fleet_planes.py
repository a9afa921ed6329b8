#!/usr/bin/env python3
"""Throughput of fleet separation on one GPU: the predicted collision points (rmpc_fleet_points_device, boxer rule)
and the separating planes (rmpc_fleet_planes_device, an all-pairs scan of B^2 N pair tests), N = 30 stages,
B = 256, 1024 and 4096 robots, K = 4 and 8 neighbours, range +inf (every robot a candidate: the scan's worst case).
Robots are spread uniformly over a square that holds 4 robots per 10 m^2, whatever B.

  - times are medians of --reps event-timed launches (each synchronised), after one warm-up launch;
  - pair tests/s = B^2 N over the planes launch's time.

    timeout -k 10 300 python scripts/bench_fleet_planes.py [--reps 20]

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

    dev = "cuda:0"
    rng = np.random.default_rng(0)
    N, nvar = 30, 10
    res = {}
    for B in (256, 1024, 4096):
        half = 0.5 * math.sqrt(2.5 * B)
        pose = np.zeros((B, 8))
        pose[:, :2] = rng.uniform(-half, half, (B, 2))
        pose[:, 2] = rng.uniform(-math.pi, math.pi, B)
        z = np.zeros((B, N, nvar))
        z[:, :, :3] = pose[:, None, :3] + rng.normal(scale=0.05, size=(B, N, 3)) * np.arange(N)[None, :, None]
        tp, tz = torch.from_numpy(pose).to(dev), torch.from_numpy(z).to(dev)
        ef = torch.ones(B, dtype=torch.int32, device=dev)
        rad = torch.full((B,), 0.6, dtype=torch.float64, device=dev)
        pts = torch.empty((B, N, 3), dtype=torch.float64, device=dev)
        pts_ms = event_ms(lambda: _lib.fleet_points_device(tp, pts, tz, ef, 1, (0.4, 0.0), 0.0), a.reps)
        r = dict(points_ms=round(pts_ms, 4))
        for K in (4, 8):
            planes = torch.empty((B, N, K, 4), dtype=torch.float64, device=dev)
            ms = event_ms(lambda: _lib.fleet_planes_device(pts, rad, planes, K), a.reps)
            r[f"K{K}_planes_ms"] = round(ms, 4)
            r[f"K{K}_pair_tests_per_s"] = float(f"{1e3 * B * B * N / ms:.3e}")
            r[f"K{K}_step_ms"] = round(pts_ms + ms, 4)
        res[f"B{B}"] = r
    print(json.dumps(dict(bench="fleet_planes", device=torch.cuda.get_device_name(0), N=N, range="inf", results=res)))


if __name__ == "__main__":
    main()
