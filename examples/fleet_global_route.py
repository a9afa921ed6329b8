#!/usr/bin/env python3
"""Point robots (cfg2 model) crossing a store on routes from the global planner, entirely on the device -- the fleet
form of examples/boxer_example_global.py of the reference: one global path per robot at step 0
(``plan_batch``: cost-to-go fields of the distinct goals on the enlarged map, one descent per robot), then every
control step ``RouteFollower.step`` (get_local_goal: the next waypoint becomes the scene's goal) ->
``solve_scene_device`` -> ``advance_device``.  Nothing crosses PCIe between control steps; the statistics are
accumulated on the device and read once at the end.

The shelves are not constraints of the MPC (as in the reference's global example); only the margin of the enlarged map
keeps the robots away from them.  The map is enlarged as the reference does it: the values its PNG round trip yields
(``png_values``: 68/256 free, 253/256 occupied) through ``get_enlarged_obstacles`` (3 x 3 mean > 0.29 at
size_robot = 0.45), which blocks every cell next to a shelf.  Goals are 10 .. 20 m away, behind at least one shelf.

    python examples/fleet_global_route.py [--robots 256] [--steps 1200] [--seed 0] [--aisle 4] [--gap 3] [--shelf 2]
                                          [--size-robot 0.45] [--threshold 1.3]
                                          [--follower {waypoint,visible}] [--look-ahead 1.75] [--reach 16]
                                          [--sight {raw,enlarged}]

``--follower visible`` takes ``VisibleFollower`` in place of ``RouteFollower``: the goal is the farthest cell of the
route, at most ``--reach`` cells on and ``--look-ahead`` metres away, that the robot's cell sees
(include/rmpc_any_angle.h); ``--threshold`` is not used then.  ``--sight`` names the map it sees on: the
store as it is (``raw``) or the enlarged map the routes were planned on.  On the enlarged map a dense route's diagonal
step past an enlarged corner is not in line of sight, and a robot waits at such a step for good.

Prints one JSON line: arrivals at the final goal (within the fleet's ARRIVE_TOL), the control step by which 50 / 90 /
100 % of the arrivals happened, failed solves, the least clearance between a robot's centre and a raw-occupied cell
(and how many robots reached 0), ms per control step, the summed lengths of the dense routes and of the same routes
pulled tight by line of sight (``shorten_routes``) with their waypoint counts, and the robot-steps in which the visible
follower saw none of its route (``blocked``; 0 with the waypoint follower).
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

from robot_mpcs_amd.store import STORE  # noqa: E402

# the store's frame (41 x 41 cells of 0.45 m centred on the origin: inside the point robot's +-10 m joint limits)
H, W, CELL, X0, Y0 = STORE.H, STORE.W, STORE.cell, STORE.x0, STORE.y0
SIZE_ROBOT = STORE.size_robot     # k = 1: every cell that touches a shelf is blocked
LOOK_AHEAD = 1.75                 # the visible follower's default, from the sweep of DESIGN.md 28


def run(B=256, steps=1200, seed=0, dev="cuda:0", aisle=4, gap=3, size_robot=SIZE_ROBOT, threshold=1.3, shelf=2,
        follower="waypoint", look_ahead=None, reach=16, sight="raw"):
    import torch
    from robot_mpcs_amd.fleet import Arrivals, MixedFleetShard, dev_f64, limit_tensors, make_block, step_block
    from robot_mpcs_amd.global_planner import (RouteFollower, VisibleFollower, cell_xy, plan_batch, route_lengths, shelf_map,
                                               shorten_routes, store_routes)
    from robot_mpcs_amd.global_planner import png_values
    if follower not in ("waypoint", "visible") or sight not in ("raw", "enlarged"):
        raise ValueError("follower must be 'waypoint' or 'visible', sight 'raw' or 'enlarged'")
    from robot_mpcs_amd.scenarios import LIMITS, make_scenario

    rng = np.random.default_rng(seed)
    raw = shelf_map(H, W, seed=seed, aisle=aisle, gap=gap, shelf=shelf)
    g_inf, starts, goals = store_routes(raw, B, rng, X0, Y0, CELL, size_robot, dev)

    sc = make_scenario("cfg2", B=B, seed=seed)
    nob = sc.desc["nobst"]
    xinit = np.zeros((B, sc.desc["nx"]))
    xinit[:, :2] = cell_xy(starts, W, X0, Y0, CELL)
    # the scenario's round obstacles are moved out of the store: the shelves are the obstacles here
    obst = np.zeros((B, nob, 4))
    obst[:, :, 0] = 50.0 + 5.0 * np.arange(nob)
    obst[:, :, 1] = 50.0
    obst[:, :, 3] = 0.1
    goal = dev_f64(np.concatenate([xinit[:, :2], np.zeros((B, 1))], 1), dev)
    f = make_block(sc.desc, sc.setup["mpc"]["weights"], B, xinit, dev, goal=goal, r_body=dev_f64(np.full(B, 0.3), dev),
                   obst=dev_f64(obst, dev), **limit_tensors(*LIMITS["cfg2"], B, dev))
    tx, ef = f["x"], f["ef"]

    torch.cuda.synchronize()
    tp = time.perf_counter()
    paths, lens = plan_batch(g_inf, torch.from_numpy(starts).to(dev), torch.from_numpy(goals).to(dev))
    torch.cuda.synchronize()
    plan_ms = 1e3 * (time.perf_counter() - tp)
    if follower == "visible":
        seen = g_inf if sight == "enlarged" else dev_f64(png_values(raw), dev)
        follower = VisibleFollower(paths, lens, W, X0, Y0, CELL, seen, reach=reach,
                                   look_ahead=LOOK_AHEAD if look_ahead is None else look_ahead)
    else:
        follower = RouteFollower(paths, lens, W, X0, Y0, CELL, threshold=threshold)
    final = follower.final_goals()
    # the same routes pulled tight by line of sight: for the report only, the followers drive the dense ones
    short_paths, short_lens, _ = shorten_routes(g_inf, paths, lens)
    blocked = torch.zeros((), dtype=torch.int64, device=dev)
    sees = isinstance(follower, VisibleFollower)

    occ_xy = dev_f64(cell_xy(np.flatnonzero(raw.ravel() > 0.5), W, X0, Y0, CELL), dev)
    tol = MixedFleetShard.ARRIVE_TOL["cfg2"]
    fails = torch.zeros((), dtype=torch.int64, device=dev)
    clear = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    arrivals = Arrivals(B, dev)
    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    for step in range(steps):
        follower.step(tx, goal)
        if sees:
            blocked += follower.blocked.sum()
        step_block(f, previous_plan=False, flags=False)
        fails += (ef < 0).sum()
        # distance from the robot's centre to the nearest raw-occupied cell (a square of side CELL)
        d = ((tx[:, None, :2] - occ_xy[None]).abs() - 0.5 * CELL).clamp(min=0.0).norm(dim=2).min(dim=1).values
        clear = torch.minimum(clear, d)
        arrivals.update((tx[:, :2] - final).norm(dim=1) < tol, step)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / steps
    f["s"].close()
    return dict(robots=B, steps=steps, routes=int((lens > 0).sum().item()), route_len_max=int(lens.max().item()),
                plan_ms=round(plan_ms, 3), route_cells_dense=int(lens.clamp(min=0).sum().item()),
                route_cells_any_angle=int(short_lens.clamp(min=0).sum().item()),
                route_m_dense=round(float(route_lengths(paths, lens, W, CELL).sum().item()), 3),
                route_m_any_angle=round(float(route_lengths(short_paths, short_lens, W, CELL).sum().item()), 3),
                blocked_robot_steps=int(blocked.item()), **arrivals.summary(),
                failed_solves=int(fails.item()), min_clearance_m=float(clear.min().item()),
                touching=int((clear <= 0).sum().item()), clearance_p10=float(clear.quantile(0.1).item()),
                ms_per_step=round(ms, 3), arrive_tol_m=tol)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--aisle", type=int, default=4)
    ap.add_argument("--gap", type=int, default=3)
    ap.add_argument("--size-robot", type=float, default=SIZE_ROBOT)
    ap.add_argument("--threshold", type=float, default=1.3)
    ap.add_argument("--shelf", type=int, default=2)
    ap.add_argument("--follower", choices=("waypoint", "visible"), default="waypoint")
    ap.add_argument("--look-ahead", type=float, default=None, help="metres; default %s" % LOOK_AHEAD)
    ap.add_argument("--reach", type=int, default=16)
    ap.add_argument("--sight", choices=("raw", "enlarged"), default="raw")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.robots, a.steps, a.seed, aisle=a.aisle, gap=a.gap, size_robot=a.size_robot,
                         threshold=a.threshold, shelf=a.shelf, follower=a.follower, look_ahead=a.look_ahead,
                         reach=a.reach, sight=a.sight)))


if __name__ == "__main__":
    main()
