#!/usr/bin/env python3
"""Boxers crossing a store that do not know where they are: the known-map route loop of examples/fleet_store_lidar.py
with a pose estimate per robot instead of the simulator's state.  Every control step, all on one stream:

    BoxerStore.scan -> ScanMatcher.step -> RouteFollower.step(estimate) -> solve and advance -> OdometryDrift.advance

The solver keeps the simulator's state (``BoxerStore.drive``).  Each robot carries an estimate (x, y, heading) that
starts at the truth: ``OdometryDrift.advance`` integrates the noisy wheel odometry of the step onto it, and
``ScanMatcher.step`` corrects it from the ranges of the robot's own scan against the store's true map
(``rmpc_lidar_project_device`` at the believed pose, then ``rmpc_scan_match_device``).  The
``RouteFollower`` is stepped with the estimate: a robot hands over its waypoints where it believes it is.
``--dead-reckoning`` skips the matcher, ``--true-pose`` feeds the follower the truth (the loop of fleet_store_lidar.py).
Nothing crosses PCIe between control steps; the statistics stay on the device until the end.

    python examples/fleet_store_localize.py [--robots 64] [--steps 1200] [--seed 0] [--dead-reckoning | --true-pose]

Prints one JSON line: the report of the other store examples (routes, arrivals, failed solves, clearances, ms per
control step), the mean, p95 and max of the estimate's position [m] and heading [rad] error over all robot-steps and
the mean position error after the last step, and ms of ``ScanMatcher.step`` alone (median of 20 event-timed calls).
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODES = ("match", "dead-reckoning", "true-pose")


def run(B=64, steps=1200, seed=0, dev="cuda:0", K=4, rays=64, mode="match", threshold=1.3, occ_threshold=0.5):
    import torch
    from robot_mpcs_amd.fleet import Arrivals, MixedFleetShard, dev_f64, event_ms
    from robot_mpcs_amd.global_planner import plan_batch
    from robot_mpcs_amd.store import STORE as S, BoxerStore, clear_routes, store_map
    from robot_mpcs_amd.utils.localization import OdometryDrift, ScanMatcher

    if mode not in MODES:
        raise ValueError("mode: one of %s" % (MODES,))
    rng = np.random.default_rng(seed)
    g_inf, starts, goals = clear_routes(store_map(seed), B, rng, dev)
    fleet = BoxerStore(B, seed, dev, K, rays, starts, rng)
    paths, lens = plan_batch(g_inf, torch.from_numpy(starts).to(dev), torch.from_numpy(goals).to(dev))
    follower = fleet.follower(threshold, paths, lens)
    final = follower.final_goals()
    tol = MixedFleetShard.ARRIVE_TOL["cfg3"]
    arrivals = Arrivals(B, dev)
    lp = fleet.lp
    matcher = ScanMatcher(B, S.H, S.W, S.x0, S.y0, S.cell, rays, lp.max_range, lp.offset, lp.height, lp.angle_min,
                          lp.angle_max, device=dev)
    matcher.set_map(dev_f64(fleet.raw, dev), occ_threshold)
    drift = OdometryDrift(B, steps, seed)
    est = fleet.x[:, :3].clone()
    x_prev = torch.empty_like(fleet.x)
    e_pos = torch.zeros((steps, B), dtype=torch.float64, device=dev)
    e_th = torch.zeros((steps, B), dtype=torch.float64, device=dev)

    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    for step in range(steps):
        fleet.scan()
        if mode == "match":
            est.copy_(matcher.step(est, lp.ranges))
        e_pos[step] = (est[:, :2] - fleet.x[:, :2]).norm(dim=1)
        e_th[step] = (torch.remainder(est[:, 2] - fleet.x[:, 2] + math.pi, 2.0 * math.pi) - math.pi).abs()
        follower.step(fleet.x if mode == "true-pose" else est, fleet.goal)
        x_prev.copy_(fleet.x)
        ee = fleet.drive()
        drift.advance(est, x_prev, fleet.x)
        arrivals.update((ee - final).norm(dim=1) < tol, step)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / steps

    match_ms = event_ms(lambda: matcher.step(est, lp.ranges), 20)
    q = lambda e, p: float(e.flatten().quantile(p).item())
    out = dict(fleet.report(), steps=steps, mode=mode, routes=int((lens > 0).sum().item()), **arrivals.summary(),
               pos_err_mean_m=float(e_pos.mean().item()), pos_err_p95_m=q(e_pos, 0.95), pos_err_max_m=float(e_pos.max().item()),
               pos_err_final_mean_m=float(e_pos[-1].mean().item()),
               heading_err_mean_rad=float(e_th.mean().item()), heading_err_p95_rad=q(e_th, 0.95),
               heading_err_max_rad=float(e_th.max().item()),
               matched_share=float((matcher.best >= 0).double().mean().item()) if mode == "match" else None,
               ms_per_step=round(ms, 3), match_step_ms=round(match_ms, 4), arrive_tol_m=tol)
    fleet.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=64)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--threshold", type=float, default=1.3)
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--dead-reckoning", action="store_true")
    how.add_argument("--true-pose", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    mode = "dead-reckoning" if a.dead_reckoning else "true-pose" if a.true_pose else "match"
    print(json.dumps(run(a.robots, a.steps, a.seed, K=a.K, rays=a.rays, mode=mode, threshold=a.threshold)))


if __name__ == "__main__":
    main()
