#!/usr/bin/env python3
"""Point robots crossing the store of examples/fleet_global_route.py on routes from the global planner, with the shelves
as constraints of the MPC: every control step each robot gets, for every stage of the coming solve, a rectangle of free
cells of the raw map round its predicted position, written as four half-planes into the model's LinearConstraints rows
(robot_mpcs_amd.utils.corridor, include/rmpc_corridor.h).  The same map, ``store_routes``, ``plan_batch``
on the enlarged map and ``RouteFollower`` as there; the model is examples/config/fleet_pointRobotMpc.yaml with
number_obstacles = 4 + K (cfg2 has no LinearConstraints), r_body 0.3.  Every control step, all on one stream:

    RouteFollower.step -> MapCorridors.step [-> NeighbourPlanes.step] -> solve_scene_device -> advance_device(exitflag)

The corridor reads the raw map (``png_values(raw)``, threshold 0.8), not the enlarged one the routes were planned on.
``--neighbours K`` adds the separating planes against the K nearest robots in the slots behind the corridor's four.
``--no-corridor`` keeps the model and its rows and fills the four slots once with a plane far outside the store: the
baseline, the robots kept from the shelves by the enlarged map's margin alone.

    python examples/fleet_store_corridor.py [--robots 256] [--steps 1200] [--seed 0] [--reach 8] [--threshold 0.6]
                                            [--neighbours 0] [--no-corridor]

Prints one JSON line: the fields of fleet_global_route.py (arrivals at the final goal and the control step by which
50 / 90 / 100 % of them happened, failed solves, least clearance between a robot's centre and a raw-occupied cell, ms
per control step) and failed and flag-0 solves, the share of robot-steps whose solve did not converge (flags other than
1 and 2), the share of (robot, stage) seeds with status <= 0 and of those whose point lies closer than r_body to a face
of its own rectangle (the row is violated before the solve), the failed solves that had such a seed and those that had
a seed without a corridor, ``corridor_ms`` (median of 20 event-timed ``MapCorridors.step`` calls), the least clearance
over all robot-steps, over those whose solve converged and over those among them whose every stage had a corridor with
the seed r_body inside it, and the highest speed.
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

H, W, CELL, X0, Y0 = STORE.H, STORE.W, STORE.cell, STORE.x0, STORE.y0
SIZE_ROBOT = STORE.size_robot
R_BODY, HEIGHT, ARRIVE_TOL = 0.3, 0.05, 0.25      # the point robot of examples/fleet_crossing.py
FAR_PLANE = (-20.0, -20.0, 0.0, 800.0)            # the free-space decomposition's dummy plane round the origin: 28 m away
# The waypoint threshold: how far ahead the goal of a solve lies.  fleet_global_route.py takes the reference's 1.3 m; its
# robots reach 2.5 m/s there, which 1 m/s^2 cannot stop inside the 1 s horizon, and a robot that a hard plane halts faster
# than it can brake has no feasible plan (fleet_crossing.py, the lookahead note).  So the default here is that model's
# own look-ahead, ROBOTS["pointRobot"]["lookahead"] of fleet_crossing.py.  What 1.3 m gives is in DESIGN.md 29.
THRESHOLD = 0.6


def model(K):
    """(desc, mpc setup) of fleet_pointRobotMpc.yaml with 4 + K linear constraints, as fleet_crossing.py builds it"""
    from robot_mpcs_amd.models.mpcModel import normalise_descriptor
    from robot_mpcs_amd.scenarios import CONFIG_DIR, build_model
    m, setup = build_model(os.path.join(CONFIG_DIR, "fleet_pointRobotMpc.yaml"), number_obstacles=4 + K)
    return normalise_descriptor(m._model), setup


def run(B=256, steps=1200, seed=0, dev="cuda:0", corridor=True, neighbours=0, reach=8, threshold=THRESHOLD, aisle=4, gap=3, shelf=2,
        neighbour_range=3.0):
    import torch
    from robot_mpcs_amd.fleet import Arrivals, dev_f64, event_ms, limit_tensors, make_block, step_block
    from robot_mpcs_amd.global_planner import RouteFollower, cell_xy, plan_batch, png_values, shelf_map, store_routes
    from robot_mpcs_amd.scenarios import POINT_LIMITS, POINT_LIMITS_U
    from robot_mpcs_amd.utils import MapCorridors
    from robot_mpcs_amd.utils.separation import NeighbourPlanes

    K = int(neighbours)
    rng = np.random.default_rng(seed)
    raw = shelf_map(H, W, seed=seed, aisle=aisle, gap=gap, shelf=shelf)
    g_inf, starts, goals = store_routes(raw, B, rng, X0, Y0, CELL, SIZE_ROBOT, dev)
    desc, setup = model(K)
    N = desc["N"]
    xinit = np.zeros((B, desc["nx"]))
    xinit[:, :2] = cell_xy(starts, W, X0, Y0, CELL)
    rad = dev_f64(np.full(B, R_BODY), dev)
    planes = torch.zeros((B, N, 4 + K, 4), dtype=torch.float64, device=dev)
    planes[:] = torch.tensor(FAR_PLANE, dtype=torch.float64, device=dev)
    point = dict(heading=0, offset=(0.0, 0.0), height=HEIGHT)
    mc = MapCorridors(B, N, dev_f64(png_values(raw), dev), X0, Y0, CELL, occupancy_threshold=0.8, reach=reach, slot0=0,
                      planes=planes, **point) if corridor else None
    npl = NeighbourPlanes(B, N, K, range=neighbour_range, slot0=4, planes=planes, **point) if K else None
    goal = dev_f64(np.concatenate([xinit[:, :2], np.zeros((B, 1))], 1), dev)
    f = make_block(desc, setup["mpc"]["weights"], B, xinit, dev, goal=goal, r_body=rad, lin_constrs=planes,
                   **limit_tensors(POINT_LIMITS, POINT_LIMITS_U, B, dev))
    tx, z, ef = f["x"], f["z"], f["ef"]

    torch.cuda.synchronize()
    tp = time.perf_counter()
    paths, lens = plan_batch(g_inf, torch.from_numpy(starts).to(dev), torch.from_numpy(goals).to(dev))
    torch.cuda.synchronize()
    plan_ms = 1e3 * (time.perf_counter() - tp)
    follower = RouteFollower(paths, lens, W, X0, Y0, CELL, threshold=threshold)
    final = follower.final_goals()

    occ_xy = dev_f64(cell_xy(np.flatnonzero(raw.ravel() > 0.5), W, X0, Y0, CELL), dev)
    i64 = dict(dtype=torch.int64, device=dev)
    inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    fails, flag0, not_ok, no_corridor, near_face, failed_near, failed_none = (torch.zeros((), **i64) for _ in range(7))
    clear_all, clear_ok, clear_in, vmax = inf.clone(), inf.clone(), inf.clone(), torch.zeros((), dtype=torch.float64, device=dev)
    near = none = torch.zeros(B, dtype=torch.bool, device=dev)
    whole = torch.ones(B, dtype=torch.bool, device=dev)
    ever_failed = torch.zeros(B, dtype=torch.bool, device=dev)
    arrivals = Arrivals(B, dev)
    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    for step in range(steps):
        follower.step(tx, goal)
        if mc is not None:
            mc.step(tx, z if step > 0 else None, ef if step > 0 else None)
            no_corridor += (mc.status <= 0).sum()
            # seeds that start closer than r_body to a face of their own rectangle: the row is violated before the solve
            p1 = torch.cat([mc.points, torch.ones_like(mc.points[..., :1])], 2)
            face = (planes[:, :, :4, :] * p1[:, :, None, :]).sum(dim=3).min(dim=2).values
            near_seed = (mc.status == 1) & (face < R_BODY)
            near_face += near_seed.sum()
            near, none, whole = near_seed.any(dim=1), (mc.status <= 0).any(dim=1), (mc.status == 1).all(dim=1)
        if npl is not None:
            npl.step(tx, rad, z if step > 0 else None, ef if step > 0 else None)
        step_block(f, previous_plan=True, flags=True)
        ok = (ef == 1) | (ef == 2)
        fails += (ef < 0).sum()
        flag0 += (ef == 0).sum()
        not_ok += (~ok).sum()
        ever_failed |= ef < 0
        failed_near += ((ef < 0) & near).sum()
        failed_none += ((ef < 0) & none & ~near).sum()
        vmax = torch.maximum(vmax, tx[:, 3:5].norm(dim=1).max())
        # distance from the robot's centre to the nearest raw-occupied cell (a square of side CELL)
        d = ((tx[:, None, :2] - occ_xy[None]).abs() - 0.5 * CELL).clamp(min=0.0).norm(dim=2).min(dim=1).values
        clear_all = torch.minimum(clear_all, d.min())
        clear_ok = torch.minimum(clear_ok, torch.where(ok, d, inf).min())
        clear_in = torch.minimum(clear_in, torch.where(ok & whole & ~near, d, inf).min())
        arrivals.update((tx[:, :2] - final).norm(dim=1) < ARRIVE_TOL, step)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / steps
    corridor_ms = event_ms(lambda: mc.step(tx, z, ef), 20) if mc is not None else None
    seeds = B * N * steps
    out = dict(robots=B, steps=steps, seed=seed, N=N, corridor=bool(corridor), neighbours=K, reach=reach, threshold=threshold,
               r_body=R_BODY, routes=int((lens > 0).sum().item()), route_len_max=int(lens.max().item()),
               plan_ms=round(plan_ms, 3), **arrivals.summary(), failed_solves=int(fails.item()),
               flag0_solves=int(flag0.item()), not_converged_share=int(not_ok.item()) / (B * steps),
               failed_robots=int(ever_failed.sum().item()), failed_with_a_seed_near_a_face=int(failed_near.item()),
               failed_with_a_seed_without_corridor=int(failed_none.item()),
               seeds_without_corridor_share=int(no_corridor.item()) / seeds if mc is not None else None,
               seeds_near_face_share=int(near_face.item()) / seeds if mc is not None else None,
               corridor_ms=None if corridor_ms is None else round(corridor_ms, 4),
               min_clearance_m=float(clear_all.item()), min_clearance_converged_m=float(clear_ok.item()),
               min_clearance_converged_inside_m=float(clear_in.item()) if mc is not None else None,
               max_speed=float(vmax.item()), fused=f["s"].is_fused(), ms_per_step=round(ms, 3), arrive_tol_m=ARRIVE_TOL)
    f["s"].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reach", type=int, default=8)
    ap.add_argument("--threshold", type=float, default=THRESHOLD)
    ap.add_argument("--neighbours", type=int, default=0)
    ap.add_argument("--no-corridor", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.robots, a.steps, a.seed, corridor=not a.no_corridor, neighbours=a.neighbours, reach=a.reach,
                         threshold=a.threshold)))


if __name__ == "__main__":
    main()
