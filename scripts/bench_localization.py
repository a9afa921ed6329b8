#!/usr/bin/env python3
"""Time of localisation on one GPU: ``ScanMatcher.set_map`` (the edge-distance table, one launch) and
``ScanMatcher.step`` (project, then match: two launches) at B = 64, 256 and 4096 robots with R = 64 rays, for the
lattices 7 x 7 x 9 (the default) and 31 x 31 x 31 (the largest: 29 791 candidates), on the examples' store (41 x 41
cells at sub 8) and on a 128 x 128 store (sub 8 as well: a table of 1024 x 1024).  The robots stand on cells clear of
the shelves, the priors beside them; the ranges are the device's own scan.

Times are medians of --reps event-timed calls (each synchronised), after one warm-up call.

    timeout -k 10 300 python scripts/bench_localization.py [--reps 20]

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
    from robot_mpcs_amd.global_planner import shelf_map
    from robot_mpcs_amd.store import STORE, clear_cells
    from robot_mpcs_amd.utils.lidar import boxes_from_grid
    from robot_mpcs_amd.utils.localization import ScanMatcher

    dev = "cuda:0"
    rng = np.random.default_rng(0)
    rays, max_range, offset, height = 64, 10.0, (STORE.ee_offset, 0.0), 0.02
    cell = STORE.cell
    out = {}
    for H, kw in ((STORE.H, dict(aisle=STORE.aisle, shelf=STORE.shelf, gap=STORE.gap)), (128, dict(aisle=9, shelf=4, gap=6))):
        raw = shelf_map(H, H, seed=0, **kw)
        x0 = -0.5 * (H - 1) * cell
        grid = torch.from_numpy(raw.astype(np.float64)).to(dev)
        boxes = torch.from_numpy(boxes_from_grid(raw, x0, x0, cell)).to(dev)
        ok = np.flatnonzero(clear_cells(raw, 2).ravel())
        for B in (64, 256, 4096):
            cells = rng.choice(ok, B)
            true = np.zeros((B, 8))
            true[:, 0] = x0 + (cells % H) * cell + rng.uniform(-0.2, 0.2, B)
            true[:, 1] = x0 + (cells // H) * cell + rng.uniform(-0.2, 0.2, B)
            true[:, 2] = rng.uniform(-math.pi, math.pi, B)
            prior = true.copy()
            prior[:, :3] += rng.uniform(-1, 1, (B, 3)) * [0.08, 0.08, 0.03]
            d_true, d_prior = torch.from_numpy(true).to(dev), torch.from_numpy(prior).to(dev)
            points = torch.zeros((B, rays, 3), dtype=torch.float64, device=dev)
            ranges = torch.zeros((B, rays), dtype=torch.float64, device=dev)
            _lib.lidar_scan_device(d_true, points, boxes, None, max_range=max_range, offset=offset, height=height,
                                   ranges=ranges)
            for nxy, nth, step_xy, step_th in ((3, 4, 0.03, 0.01), (15, 15, 0.02, 0.005)):
                m = ScanMatcher(B, H, H, x0, x0, cell, rays, max_range, offset, height, -math.pi, math.pi, nxy=nxy,
                                step_xy=step_xy, nth=nth, step_th=step_th, device=dev)
                r = dict(set_map_ms=round(event_ms(lambda: m.set_map(grid, 0.5), a.reps), 4),
                         step_ms=round(event_ms(lambda: m.step(d_prior, ranges), a.reps), 4))
                err = (m.pose_out[:, :2] - d_true[:, :2]).norm(dim=1)
                r.update(matched=int((m.best >= 0).sum().item()), used_mean=round(float(m.used.double().mean().item()), 1),
                         pos_err_mean_m=round(float(err.mean().item()), 4), pos_err_max_m=round(float(err.max().item()), 4))
                out[f"{H}x{H}_B{B}_{2 * nxy + 1}x{2 * nxy + 1}x{2 * nth + 1}"] = r
    print(json.dumps(dict(bench="localization", device=torch.cuda.get_device_name(0), reps=a.reps, rays=rays, sub=8,
                          cap=256, cases=out)))


if __name__ == "__main__":
    main()
