#!/usr/bin/env python3
"""Boxers crossing a store with a lidar, entirely on the device -- the fleet form of the reference's
examples/boxer_example_supermarket.py.  Every robot gets one global route at step 0 (``plan_batch`` on the store's map
enlarged by one cell, as examples/fleet_global_route.py does).  Then every control step, all on one stream:

    RouteFollower.step -> LidarPlanes.step -> solve_scene_device -> advance_device(..., exitflag=ef)

``LidarPlanes.step`` scans the shelves (64 rays, a full circle: a boxer turns in place), seeds one free-space
decomposition per stage at the sensor position of that stage in the previous plan (the current pose on the first
step and after a failed solve) and writes K planes per stage into the scene's ``lin_constrs``: the boxer's shipped
LinearConstraints model (boxerMpc.yaml, ``make_scenario("boxer", number_obstacles=K)``) keeps its end link r_body from
every plane.  Nothing crosses PCIe between control steps; the statistics stay on the device until the end.

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
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# the store: 41 x 41 cells of 0.45 m centred on the origin (inside the boxer's +-10 m position limits); aisles of
# 6 cells (2.7 m) and passages of 5 cells through the shelves, for a body of r_body = 0.6 m around the end link
H = W = 41
CELL = 0.45
X0 = Y0 = -9.0
AISLE, SHELF, GAP = 6, 2, 5
SIZE_ROBOT = 0.45     # k = 1, as in fleet_global_route.py: the route alone does not keep r_body clear
R_BODY = 0.6
EE_OFFSET = 0.4       # ee_link ahead of base_link (boxer_fk.urdf); the lidar sits there too (compute_point_cloud)
# starts and goals: no shelf cell within this many cells (Chebyshev), i.e. >= 1.125 m from a shelf's edge, so that the
# end link starts outside r_body of every shelf whatever the heading
CLEAR_CELLS = 2


def clear_cells(raw, k):
    """free cells with no occupied cell within Chebyshev distance k"""
    occ = np.pad(raw > 0.5, k, constant_values=True)
    near = np.zeros(raw.shape, dtype=bool)
    for dr in range(-k, k + 1):
        for dc in range(-k, k + 1):
            near |= occ[k + dr:k + dr + H, k + dc:k + dc + W]
    return ~near


def box_distance(p, boxes):
    """(B,) least distance from the points p (B, 2) to the boxes (nbox, 4) = (cx, cy, lx, ly); 0 inside"""
    return ((p[:, None, :] - boxes[None, :, :2]).abs() - 0.5 * boxes[None, :, 2:]).clamp(min=0.0).norm(dim=2).min(dim=1).values


def run(B=256, steps=1200, seed=0, dev="cuda:0", K=4, rays=64, lidar=True, threshold=1.3):
    import torch
    from robot_mpcs_amd.fleet import (Arrivals, MixedFleetShard, dev_f64, event_ms, limit_tensors, make_block,
                                      step_block)
    from robot_mpcs_amd.global_planner import RouteFollower, cell_xy, plan_batch, shelf_map, store_routes
    from robot_mpcs_amd.scenarios import LIMITS, make_scenario
    from robot_mpcs_amd.utils.lidar import LidarPlanes, boxes_from_grid

    rng = np.random.default_rng(seed)
    raw = shelf_map(H, W, seed=seed, aisle=AISLE, gap=GAP, shelf=SHELF)
    g_inf, starts, goals = store_routes(raw, B, rng, X0, Y0, CELL, SIZE_ROBOT, dev, ok=clear_cells(raw, CLEAR_CELLS))
    boxes_np = boxes_from_grid(raw, X0, Y0, CELL)
    boxes = dev_f64(boxes_np, dev)

    sc = make_scenario("boxer", B=B, seed=seed, number_obstacles=K)
    xinit = np.zeros((B, sc.desc["nx"]))
    xinit[:, :2] = cell_xy(starts, W, X0, Y0, CELL)
    xinit[:, 2] = rng.uniform(-math.pi, math.pi, B)
    lp = LidarPlanes(B, sc.desc["N"], K, boxes=boxes_np if lidar else None, rays=rays, offset=(EE_OFFSET, 0.0), device=dev)
    goal = dev_f64(np.concatenate([xinit[:, :2], np.zeros((B, 1))], 1), dev)
    f = make_block(sc.desc, sc.setup["mpc"]["weights"], B, xinit, dev, goal=goal, r_body=dev_f64(np.full(B, R_BODY), dev),
                   lin_constrs=lp.planes, **limit_tensors(*LIMITS["boxer"], B, dev))
    tx, z, ef = f["x"], f["z"], f["ef"]

    paths, lens = plan_batch(g_inf, torch.from_numpy(starts).to(dev), torch.from_numpy(goals).to(dev))
    follower = RouteFollower(paths, lens, W, X0, Y0, CELL, threshold=threshold)
    final = follower.final_goals()

    tol = MixedFleetShard.ARRIVE_TOL["cfg3"]
    fails = torch.zeros((), dtype=torch.int64, device=dev)
    ee_clear = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    base_clear = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    arrivals = Arrivals(B, dev)

    def ee_of(x):
        return x[:, :2] + EE_OFFSET * torch.stack([torch.cos(x[:, 2]), torch.sin(x[:, 2])], 1)

    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    for step in range(steps):
        follower.step(tx, goal)
        lp.step(tx, z if step > 0 else None, ef if step > 0 else None)
        step_block(f, previous_plan=True)
        fails += (ef < 0).sum()
        ee = ee_of(tx)
        ee_clear = torch.minimum(ee_clear, box_distance(ee, boxes))
        base_clear = torch.minimum(base_clear, box_distance(tx[:, :2], boxes))
        arrivals.update((ee - final).norm(dim=1) < tol, step)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / steps

    lidar_ms = event_ms(lambda: lp.step(tx, z, ef), 20)
    out = dict(robots=B, steps=steps, K=K, rays=rays, lidar=bool(lidar), fused=f["s"].is_fused(), nbox=int(len(boxes_np)),
               routes=int((lens > 0).sum().item()), **arrivals.summary(),
               failed_solves=int(fails.item()), failed_share=int(fails.item()) / (B * steps),
               min_ee_clearance_m=float(ee_clear.min().item()), ee_clearance_p10=float(ee_clear.quantile(0.1).item()),
               ee_below_half_r_body=int((ee_clear < 0.5 * R_BODY).sum().item()),
               min_base_clearance_m=float(base_clear.min().item()), base_inside=int((base_clear <= 0).sum().item()),
               ms_per_step=round(ms, 3), lidar_step_ms=round(lidar_ms, 4), arrive_tol_m=tol, r_body=R_BODY)
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
    ap.add_argument("--no-lidar", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.robots, a.steps, a.seed, K=a.K, rays=a.rays, lidar=not a.no_lidar, threshold=a.threshold)))


if __name__ == "__main__":
    main()
