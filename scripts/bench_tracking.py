#!/usr/bin/env python3
"""Time of the moving-obstacle tracker on one GPU: ``rmpc_lidar_tracks_device`` alone and the whole
``ObstacleTracker.step`` (the scan of the walkers, the sensor origins, the tracker: three launches without boxes) at
B = 64, 256 and 4096 robots with R = 64, 256 and 1024 rays, among 24 walkers of radius 0.3 m in a +-9 m arena.  The
tracker is warmed by ten steps of the moving walkers, so that its slots hold confirmed tracks when it is timed.

Times are medians of --reps event-timed calls (each synchronised), after one warm-up call.

    timeout -k 10 300 python scripts/bench_tracking.py [--reps 20]

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
    from robot_mpcs_amd.utils.tracking import ObstacleTracker

    dev = "cuda:0"
    rng = np.random.default_rng(0)
    P, dt = 24, 0.1
    out = {}
    for B in (64, 256, 4096):
        pose = np.zeros((B, 8))
        pose[:, :2] = rng.uniform(-6, 6, (B, 2))
        pose[:, 2] = rng.uniform(-math.pi, math.pi, B)
        d_pose = torch.from_numpy(pose).to(dev)
        w = np.concatenate([rng.uniform(-8, 8, (P, 2)), rng.uniform(-0.5, 0.5, (P, 2))], axis=1)
        for R in (64, 256, 1024):
            trk = ObstacleTracker(B, 5, rays=R, n_tracks=8, radius=0.3, dt=dt, device=dev)
            circles = torch.full((P, 3), 0.3, dtype=torch.float64, device=dev)
            for k in range(10):
                circles[:, :2] = torch.from_numpy(w[:, :2] + k * dt * w[:, 2:]).to(dev)
                trk.step(d_pose, circles)
            r = dict(tracks_ms=round(event_ms(lambda: _lib.lidar_tracks_device(trk.args, B), a.reps), 4),
                     step_ms=round(event_ms(lambda: trk.step(d_pose, circles), a.reps), 4))
            c = trk.counts.double().mean(dim=0).cpu().numpy()
            r.update(segments_mean=round(float(c[0]), 2), detections_mean=round(float(c[1]), 2),
                     live_mean=round(float(c[2]), 2), confirmed_mean=round(float(c[3]), 2))
            out[f"B{B}_R{R}"] = r
    print(json.dumps(dict(bench="tracking", device=torch.cuda.get_device_name(0), reps=a.reps, walkers=P, n_tracks=8,
                          n_out=5, cases=out)))


if __name__ == "__main__":
    main()
