#!/usr/bin/env python3
"""Boxers crossing a store they have no map of: the loop of examples/fleet_store_lidar.py (same store, seed, starts,
goals, constants and ``LidarPlanes``: ``BoxerStore`` of robot_mpcs_amd/store.py), but the global planner starts with an empty map, the fleet marks every scan into
a shared occupancy map (``FleetMap``: rmpc_grid_mark_device) and re-plans its routes on what it has seen so far.
Every control step, all on one stream:

    RouteFollower.step -> LidarPlanes.step -> FleetMap.mark -> solve_scene_device -> advance_device(..., exitflag=ef)

and at step 0 and every ``--replan-every`` steps, before it:

    FleetMap.occupancy(68/256, 253/256, 68/256) -> grid_inflate_device -> replan

The three values are those of the reference's PNG round trip (``png_values``); unknown space gets the free value, so
routes are planned through what nobody has seen yet and move out of a shelf once a scan has found it.  A robot whose
own cell is occupied on the enlarged map keeps the route it has.  ``--known-map`` is the loop of
examples/fleet_store_lidar.py, one plan on the store's true map, for comparison.

    python examples/fleet_store_explore.py [--robots 256] [--steps 1200] [--seed 0] [--replan-every 10] [--known-map]

Prints one JSON line: the fields of examples/fleet_store_lidar.py (``routes`` = the robots that hold a route at the
end), the cells of the map with evidence and those among them whose class differs from the true map, the number of
re-plans, and ms of ``FleetMap.mark``, ``FleetMap.occupancy`` and ``replan`` (medians of 20 event-timed calls).
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


def run(B=256, steps=1200, seed=0, dev="cuda:0", K=4, rays=64, threshold=1.3, replan_every=10, known_map=False):
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import Arrivals, MixedFleetShard, dev_f64, event_ms
    from robot_mpcs_amd.global_planner import FREE, OCC, cell_xy, plan_batch, replan
    from robot_mpcs_amd.store import STORE, BoxerStore, clear_routes, map_errors, store_map

    rng = np.random.default_rng(seed)
    g_inf, starts, goals = clear_routes(store_map(seed), B, rng, dev)
    fleet = BoxerStore(B, seed, dev, K, rays, starts, rng)
    lp, tx = fleet.lp, fleet.x

    goal_cells = torch.from_numpy(goals).to(dev)
    final = dev_f64(cell_xy(goals, STORE.W, STORE.x0, STORE.y0, STORE.cell), dev)
    if known_map:
        follower = fleet.follower(threshold, *plan_batch(g_inf, torch.from_numpy(starts).to(dev), goal_cells))
    else:
        fmap = fleet.fleet_map()
        g_obs = torch.empty((STORE.H, STORE.W), dtype=torch.float64, device=dev)
        follower = fleet.follower(threshold)

    def plan_on_seen():
        _lib.grid_inflate_device(fmap.occupancy(FREE, OCC, FREE), g_obs, STORE.cell, STORE.size_robot, 0.29)
        return replan(follower, g_obs, tx, goal_cells)

    tol = MixedFleetShard.ARRIVE_TOL["cfg3"]
    arrivals = Arrivals(B, dev)
    replans = 0

    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    for step in range(steps):
        if not known_map and step % replan_every == 0:
            plan_on_seen()
            replans += 1
        follower.step(tx, fleet.goal)
        fleet.scan()
        if not known_map:
            fmap.mark(tx, lp.points, lp.ranges)
        ee = fleet.drive()
        arrivals.update((ee - final).norm(dim=1) < tol, step)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / steps

    routes = int((follower.lens > 0).sum().item())
    lidar_ms = event_ms(fleet.scan, 20)
    extra = dict(map_seen_cells=None, map_wrong_cells=None, replans=replans, mark_ms=None, occupancy_ms=None,
                 replan_ms=None)
    if not known_map:
        extra["map_seen_cells"], extra["map_wrong_cells"] = map_errors(fmap, fleet.raw)
        extra.update(mark_ms=round(event_ms(lambda: fmap.mark(tx, lp.points, lp.ranges), 20), 4),
                     occupancy_ms=round(event_ms(lambda: fmap.occupancy(FREE, OCC, FREE), 20), 4),
                     replan_ms=round(event_ms(plan_on_seen, 20), 4))
    out = dict(fleet.report(), steps=steps, lidar=True, routes=routes, **arrivals.summary(), ms_per_step=round(ms, 3),
               lidar_step_ms=round(lidar_ms, 4), arrive_tol_m=tol, **extra)
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
    ap.add_argument("--replan-every", type=int, default=10)
    ap.add_argument("--known-map", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.robots, a.steps, a.seed, K=a.K, rays=a.rays, threshold=a.threshold,
                         replan_every=a.replan_every, known_map=a.known_map)))


if __name__ == "__main__":
    main()
