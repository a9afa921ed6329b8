#!/usr/bin/env python3
"""Boxers crossing a store with a lidar, entirely on the device -- the fleet form of the reference's
examples/boxer_example_supermarket.py.  Every robot gets one global route at step 0 (``plan_batch`` on the store's map
enlarged by one cell, as examples/fleet_global_route.py does).  Then every control step, all on one stream:

    RouteFollower.step -> LidarPlanes.step -> solve_scene_device -> advance_device(..., exitflag=ef)

``LidarPlanes.step`` scans the shelves (64 rays, a full circle: a boxer turns in place), seeds one free-space
decomposition per stage at the sensor position of that stage in the previous plan (the current pose on the first
step and after a failed solve) and writes K planes per stage into the scene's ``lin_constrs``: the boxer's shipped
LinearConstraints model (boxerMpc.yaml, ``make_scenario("boxer", number_obstacles=K)``) keeps its end link r_body from
every plane.  Nothing crosses PCIe between control steps; the statistics stay on the device until the end.  The fleet,
its block and its statistics are ``BoxerStore`` of robot_mpcs_amd/store.py, which the other store examples share.

The map's enlargement alone does not keep r_body = 0.6 m clear: a route may pass 0.225 m from a shelf's edge.  With
``--no-lidar`` the planes stay at the free-space decomposition's dummy planes (every ray misses an empty world): the
A/B baseline in which only the route keeps the robots off the shelves.

    python examples/fleet_store_lidar.py [--robots 256] [--steps 1200] [--seed 0] [--K 4] [--rays 64] [--no-lidar]

Prints one JSON line: routes found, arrivals (the end link within ARRIVE_TOL["cfg3"] of the final goal) and the control
step by which 50 / 90 / 100 % of them happened, failed solves, the least distance from the end link and from the base
centre to any shelf box, whether the chosen K runs on the fused kernel, ms per control step and ms of
``LidarPlanes.step`` alone (median of 20 event-timed calls).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run(B=256, steps=1200, seed=0, dev="cuda:0", K=4, rays=64, lidar=True, threshold=1.3):
    import torch
    from robot_mpcs_amd.fleet import Arrivals, MixedFleetShard, event_ms
    from robot_mpcs_amd.global_planner import plan_batch
    from robot_mpcs_amd.store import BoxerStore, clear_routes, store_map

    rng = np.random.default_rng(seed)
    g_inf, starts, goals = clear_routes(store_map(seed), B, rng, dev)
    fleet = BoxerStore(B, seed, dev, K, rays, starts, rng, lidar=lidar)
    paths, lens = plan_batch(g_inf, torch.from_numpy(starts).to(dev), torch.from_numpy(goals).to(dev))
    follower = fleet.follower(threshold, paths, lens)
    final = follower.final_goals()
    tol = MixedFleetShard.ARRIVE_TOL["cfg3"]
    arrivals = Arrivals(B, dev)

    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    for step in range(steps):
        follower.step(fleet.x, fleet.goal)
        fleet.scan()
        ee = fleet.drive()
        arrivals.update((ee - final).norm(dim=1) < tol, step)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / steps

    lidar_ms = event_ms(fleet.scan, 20)
    out = dict(fleet.report(), steps=steps, lidar=bool(lidar), routes=int((lens > 0).sum().item()), **arrivals.summary(),
               ms_per_step=round(ms, 3), lidar_step_ms=round(lidar_ms, 4), arrive_tol_m=tol)
    fleet.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--threshold", type=float, default=1.3)
    ap.add_argument("--no-lidar", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.robots, a.steps, a.seed, K=a.K, rays=a.rays, lidar=not a.no_lidar, threshold=a.threshold)))


if __name__ == "__main__":
    main()
