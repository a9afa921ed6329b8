#!/usr/bin/env python3
"""Boxers crossing a store they have no map of: the loop of examples/fleet_store_lidar.py (same store, seed, starts,
goals, constants and ``LidarPlanes``), but the global planner starts with an empty map, the fleet marks every scan into
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
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import fleet_store_lidar as store  # noqa: E402  (the store, its constants and helpers)

FREE, OCC = 68.0 / 256.0, 253.0 / 256.0    # png_values: what grid_inflate_device gets in the reference


def run(B=256, steps=1200, seed=0, dev="cuda:0", K=4, rays=64, threshold=1.3, replan_every=10, known_map=False):
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import (Arrivals, MixedFleetShard, dev_f64, event_ms, limit_tensors, make_block,
                                      step_block)
    from robot_mpcs_amd.global_planner import RouteFollower, cell_xy, plan_batch, replan, shelf_map, store_routes
    from robot_mpcs_amd.scenarios import LIMITS, make_scenario
    from robot_mpcs_amd.utils.lidar import LidarPlanes, boxes_from_grid
    from robot_mpcs_amd.utils.mapping import FleetMap

    H, W, CELL, X0, Y0 = store.H, store.W, store.CELL, store.X0, store.Y0
    rng = np.random.default_rng(seed)
    raw = shelf_map(H, W, seed=seed, aisle=store.AISLE, gap=store.GAP, shelf=store.SHELF)
    g_inf, starts, goals = store_routes(raw, B, rng, X0, Y0, CELL, store.SIZE_ROBOT, dev,
                                        ok=store.clear_cells(raw, store.CLEAR_CELLS))
    boxes_np = boxes_from_grid(raw, X0, Y0, CELL)
    boxes = dev_f64(boxes_np, dev)

    sc = make_scenario("boxer", B=B, seed=seed, number_obstacles=K)
    xinit = np.zeros((B, sc.desc["nx"]))
    xinit[:, :2] = cell_xy(starts, W, X0, Y0, CELL)
    xinit[:, 2] = rng.uniform(-math.pi, math.pi, B)
    lp = LidarPlanes(B, sc.desc["N"], K, boxes=boxes_np, rays=rays, offset=(store.EE_OFFSET, 0.0), device=dev)
    goal = dev_f64(np.concatenate([xinit[:, :2], np.zeros((B, 1))], 1), dev)
    f = make_block(sc.desc, sc.setup["mpc"]["weights"], B, xinit, dev, goal=goal,
                   r_body=dev_f64(np.full(B, store.R_BODY), dev), lin_constrs=lp.planes,
                   **limit_tensors(*LIMITS["boxer"], B, dev))
    tx, z, ef = f["x"], f["z"], f["ef"]

    goal_cells = torch.from_numpy(goals).to(dev)
    final = dev_f64(cell_xy(goals, W, X0, Y0, CELL), dev)
    if known_map:
        paths, lens = plan_batch(g_inf, torch.from_numpy(starts).to(dev), goal_cells)
        follower = RouteFollower(paths, lens, W, X0, Y0, CELL, threshold=threshold)
    else:
        fmap = FleetMap(B, H, W, X0, Y0, CELL, rays, lp.max_range, lp.offset, lp.height, device=dev)
        g_obs = torch.empty((H, W), dtype=torch.float64, device=dev)
        max_len = min(H * W, 4 * (H + W))     # plan_batch's default: replace() then never has to pad
        follower = RouteFollower(torch.zeros((B, max_len), dtype=torch.int32, device=dev),
                                 torch.zeros(B, dtype=torch.int32, device=dev), W, X0, Y0, CELL, threshold=threshold)

    def plan_on_seen():
        _lib.grid_inflate_device(fmap.occupancy(FREE, OCC, FREE), g_obs, CELL, store.SIZE_ROBOT, 0.29)
        return replan(follower, g_obs, tx, goal_cells)

    tol = MixedFleetShard.ARRIVE_TOL["cfg3"]
    fails = torch.zeros((), dtype=torch.int64, device=dev)
    ee_clear = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    base_clear = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    arrivals = Arrivals(B, dev)
    replans = 0

    def ee_of(x):
        return x[:, :2] + store.EE_OFFSET * torch.stack([torch.cos(x[:, 2]), torch.sin(x[:, 2])], 1)

    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    for step in range(steps):
        if not known_map and step % replan_every == 0:
            plan_on_seen()
            replans += 1
        follower.step(tx, goal)
        lp.step(tx, z if step > 0 else None, ef if step > 0 else None)
        if not known_map:
            fmap.mark(tx, lp.points, lp.ranges)
        step_block(f, previous_plan=True)
        fails += (ef < 0).sum()
        ee = ee_of(tx)
        ee_clear = torch.minimum(ee_clear, store.box_distance(ee, boxes))
        base_clear = torch.minimum(base_clear, store.box_distance(tx[:, :2], boxes))
        arrivals.update((ee - final).norm(dim=1) < tol, step)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / steps

    extra = dict(map_seen_cells=None, map_wrong_cells=None, replans=replans, mark_ms=None, occupancy_ms=None,
                 replan_ms=None)
    if not known_map:
        seen = (fmap.hits.long() + fmap.misses.long()) > 0
        truth = torch.from_numpy(raw > 0.5).to(dev)
        wrong = seen & ((fmap.occupancy(0.0, 1.0, 0.0) > 0.5) != truth)
        extra.update(map_seen_cells=int(seen.sum().item()), map_wrong_cells=int(wrong.sum().item()))
    routes = int((follower.lens > 0).sum().item())
    lidar_ms = event_ms(lambda: lp.step(tx, z, ef), 20)
    if not known_map:
        extra.update(mark_ms=round(event_ms(lambda: fmap.mark(tx, lp.points, lp.ranges), 20), 4),
                     occupancy_ms=round(event_ms(lambda: fmap.occupancy(FREE, OCC, FREE), 20), 4),
                     replan_ms=round(event_ms(plan_on_seen, 20), 4))
    out = dict(robots=B, steps=steps, K=K, rays=rays, lidar=True,
               fused=f["s"].is_fused(), nbox=int(len(boxes_np)), routes=routes, **arrivals.summary(),
               failed_solves=int(fails.item()), failed_share=int(fails.item()) / (B * steps),
               min_ee_clearance_m=float(ee_clear.min().item()), ee_clearance_p10=float(ee_clear.quantile(0.1).item()),
               ee_below_half_r_body=int((ee_clear < 0.5 * store.R_BODY).sum().item()),
               min_base_clearance_m=float(base_clear.min().item()), base_inside=int((base_clear <= 0).sum().item()),
               ms_per_step=round(ms, 3), lidar_step_ms=round(lidar_ms, 4), arrive_tol_m=tol, r_body=store.R_BODY, **extra)
    f["s"].close()
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
