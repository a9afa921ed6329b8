#!/usr/bin/env python3
"""Boxers crossing a store far beyond the 128 x 128 cells one workgroup's LDS holds: 301 x 301 cells of 0.45 m (135 m on
a side), routes from the global planner on the device.  The prologue is that of examples/fleet_global_route.py --
``store_routes`` (the map enlarged as the reference does it, starts and goals 10 .. 20 m apart behind a shelf) ->
``plan_batch``, which on a map of this size takes ``rmpc_grid_fields_large_device`` -> ``RouteFollower``
-> ``make_block`` / ``step_block`` -- with the boxer's shipped LinearConstraints model (boxerMpc.yaml, K planes) whose
lidar looks into an empty world, as ``BoxerStore(lidar=False)`` does in the 41 x 41 store: the route alone keeps the
robots off the shelves.  The boxer's position limits are widened to the store.

    python examples/fleet_large_store.py [--robots 256] [--steps 1200] [--seed 0] [--side 301] [--K 4]

Prints one JSON line: the plan's time (fields and descents, synchronised), the routes found and their lengths in cells,
arrivals (the end link within ARRIVE_TOL["cfg3"] of the final goal) with the control steps by which 50 / 90 / 100 % of
them happened, failed solves and ms per control step.  Reported, not gated.
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

from robot_mpcs_amd.store import STORE, clear_cells  # noqa: E402


def run(B=256, steps=1200, seed=0, dev="cuda:0", side=301, K=4, threshold=1.3):
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import Arrivals, MixedFleetShard, dev_f64, limit_tensors, make_block, step_block
    from robot_mpcs_amd.global_planner import RouteFollower, cell_xy, plan_batch, shelf_map, store_routes
    from robot_mpcs_amd.scenarios import LIMITS, make_scenario
    from robot_mpcs_amd.utils.lidar import LidarPlanes

    S = STORE
    H = W = int(side)
    x0 = y0 = -0.5 * (side - 1) * S.cell                 # the store centred on the origin
    rng = np.random.default_rng(seed)
    raw = shelf_map(H, W, seed=seed, aisle=S.aisle, gap=S.gap, shelf=S.shelf)
    g_inf, starts, goals = store_routes(raw, B, rng, x0, y0, S.cell, S.size_robot, dev, ok=clear_cells(raw, S.clear_cells))

    torch.cuda.synchronize()
    tp = time.perf_counter()
    paths, lens = plan_batch(g_inf, torch.from_numpy(starts).to(dev), torch.from_numpy(goals).to(dev))
    torch.cuda.synchronize()
    plan_ms = 1e3 * (time.perf_counter() - tp)
    follower = RouteFollower(paths, lens, W, x0, y0, S.cell, threshold=threshold)
    final = follower.final_goals()

    sc = make_scenario("boxer", B=B, seed=seed, number_obstacles=K)
    xinit = np.zeros((B, sc.desc["nx"]))
    xinit[:, :2] = cell_xy(starts, W, x0, y0, S.cell)
    xinit[:, 2] = rng.uniform(-math.pi, math.pi, B)
    lim, limu = (a.copy() for a in LIMITS["boxer"])
    lim[0, :2], lim[1, :2] = x0 - 1.0, -x0 + 1.0         # the boxer's +-10 m position limits, widened to the store
    lp = LidarPlanes(B, sc.desc["N"], K, boxes=None, rays=64, offset=(S.ee_offset, 0.0), device=dev)
    goal = dev_f64(np.concatenate([xinit[:, :2], np.zeros((B, 1))], 1), dev)
    f = make_block(sc.desc, sc.setup["mpc"]["weights"], B, xinit, dev, goal=goal, r_body=dev_f64(np.full(B, S.r_body), dev),
                   lin_constrs=lp.planes, **limit_tensors(lim, limu, B, dev))
    x, z, ef = f["x"], f["z"], f["ef"]

    tol = MixedFleetShard.ARRIVE_TOL["cfg3"]
    fails = torch.zeros((), dtype=torch.int64, device=dev)
    arrivals = Arrivals(B, dev)
    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    for step in range(steps):
        follower.step(x, goal)
        lp.step(x, *((None, None) if step == 0 else (z, ef)))
        step_block(f, previous_plan=True)
        fails += (ef < 0).sum()
        ee = x[:, :2] + S.ee_offset * torch.stack([torch.cos(x[:, 2]), torch.sin(x[:, 2])], 1)
        arrivals.update((ee - final).norm(dim=1) < tol, step)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / max(steps, 1)
    f["s"].close()
    L = lens.cpu().numpy()
    return dict(robots=B, steps=steps, map="%dx%d" % (H, W), cell_m=S.cell, cells=H * W, lds_entry_max_cells=_lib.GRID_MAX_CELLS,
                distinct_goals=int(len(np.unique(goals))), plan_ms=round(plan_ms, 3), routes=int((L > 0).sum()),
                route_len_min=int(L[L > 0].min()) if (L > 0).any() else 0, route_len_max=int(L.max()),
                route_len_mean=round(float(L[L > 0].mean()), 1) if (L > 0).any() else 0.0, **arrivals.summary(),
                failed_solves=int(fails.item()), ms_per_step=round(ms, 3), arrive_tol_m=tol)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--side", type=int, default=301)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--threshold", type=float, default=1.3)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.robots, a.steps, a.seed, side=a.side, K=a.K, threshold=a.threshold)))


if __name__ == "__main__":
    main()
