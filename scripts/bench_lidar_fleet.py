#!/usr/bin/env python3
"""The fleet in the scan on one GPU (rmpc_lidar_scan_fleet_device) against the workaround it replaces:
the same robots appended as circles to the plain scan (rmpc_lidar_scan_device).  Bodies of radius 0.3 .. 0.6 m are
centred on the sensors, so both give one answer (checked on every row: equal ranges).

  - B = P in {64, 256, 1024, 4096} robots, R in {64, 256} rays, range 10 m, on a square floor of about 5 m^2 per robot
    (the density of examples/fleet_crossing.py: +-72 m at 4096) with 60 boxes and 5 circles;
  - one dense row: 1024 robots within +-3 m, every body in range of every robot;
  - times are medians of --reps event-timed calls (each synchronised), after one warm call;
  - per row: both times, their ratio, and the bodies in range of a robot (min / median / max).

    timeout -k 10 300 python scripts/bench_lidar_fleet.py [--reps 20]

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

RANGE, OFFSET, NBOX, NCIRCLE = 10.0, (0.4, 0.0), 60, 5


def world(rng, B, arena):
    """pose (B, 8), boxes, circles of the floor, radius (B,); box sides are 1 .. 10 % of the arena's half-width"""
    pose = np.zeros((B, 8))
    pose[:, :2] = rng.uniform(-arena, arena, (B, 2))
    pose[:, 2] = rng.uniform(-math.pi, math.pi, B)
    boxes = np.concatenate([rng.uniform(-arena, arena, (NBOX, 2)), rng.uniform(0.01, 0.1, (NBOX, 2)) * arena], 1)
    circles = np.concatenate([rng.uniform(-arena, arena, (NCIRCLE, 2)), rng.uniform(0.02, 0.08, (NCIRCLE, 1)) * arena], 1)
    return pose, boxes, circles, rng.uniform(0.3, 0.6, B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import dev_f64, event_ms

    dev = "cuda:0"
    rng = np.random.default_rng(0)
    rows = []
    runs = [(B, R, math.sqrt(5.0 * B) / 2.0, False) for B in (64, 256, 1024, 4096) for R in (64, 256)]
    runs.append((1024, 64, 3.0, True))
    for B, R, arena, dense in runs:
        pose_np, boxes_np, circles_np, radius_np = world(rng, B, arena)
        pose, boxes, radius = dev_f64(pose_np, dev), dev_f64(boxes_np, dev), dev_f64(radius_np, dev)
        circles = dev_f64(circles_np, dev)
        centres = torch.zeros((B, 1, 3), dtype=torch.float64, device=dev)
        _lib.fleet_points_device(pose, centres, None, None, 1, OFFSET, 0.0)          # the sensors' positions
        appended = torch.cat([circles, torch.cat([centres[:, 0, :2], radius[:, None]], 1)], 0).contiguous()
        pts, rng_ = (torch.zeros((B, R, 3), dtype=torch.float64, device=dev),
                     torch.zeros((B, R), dtype=torch.float64, device=dev))
        pts2, rng2 = torch.zeros_like(pts), torch.zeros_like(rng_)
        own = torch.zeros((B, R), dtype=torch.int32, device=dev)
        fleet = lambda: _lib.lidar_scan_fleet_device(pose, pts, centres, radius, boxes, circles, max_range=RANGE,
                                                     offset=OFFSET, owner=own, ranges=rng_)
        plain = lambda: _lib.lidar_scan_device(pose, pts2, boxes, appended, max_range=RANGE, offset=OFFSET, ranges=rng2)
        fleet_ms, plain_ms = event_ms(fleet, a.reps), event_ms(plain, a.reps)
        torch.cuda.synchronize()
        c = centres[:, 0, :2]
        d = (c[:, None, :] - c[None, :, :]).norm(dim=2)
        d.fill_diagonal_(float("inf"))
        n = (d <= RANGE + radius[None, :]).sum(dim=1).cpu().numpy()
        rows.append(dict(B=B, R=R, arena_m=round(arena, 2), dense=dense, fleet_ms=round(fleet_ms, 4),
                         circles_ms=round(plain_ms, 4), circles_over_fleet=round(plain_ms / fleet_ms, 2),
                         in_range_min=int(n.min()), in_range_median=float(np.median(n)), in_range_max=int(n.max()),
                         body_ray_share=round(float((own >= 0).double().mean().item()), 4),
                         same_ranges=bool(torch.equal(rng_, rng2))))
    print(json.dumps(dict(bench="lidar_fleet", device=torch.cuda.get_device_name(0), range_m=RANGE, reps=a.reps, rows=rows)))


if __name__ == "__main__":
    main()
