#!/usr/bin/env python3
"""Boxers sent to a set of pick cells in a store, entirely on the device: who goes where is decided
first, then the loop of examples/fleet_store_lidar.py drives the routes.  B boxers on random clear cells, T >= B random
clear pick cells, and one of three pairings on the same B x T route costs (``GoalAssigner``: one cost-to-go field per
pick cell, ``rmpc_grid_route_costs_device``):

    fixed    robot b goes to pick cell b
    greedy   rmpc_assign_greedy_device: the least (cost, b, t) pair first
    optimal  rmpc_assign_optimal_device: the least sum of route costs (include/rmpc_assign_opt.h)

    RouteFollower.step -> LidarPlanes.step -> solve_scene_device -> advance_device(..., exitflag=ef)

    python examples/fleet_store_dispatch.py [--robots 16] [--goals 24] [--steps 400] [--seed 0]
                                            [--assign fixed|greedy|optimal]

Prints one JSON line: the report fields of the store examples, the sum of the route costs of the pairing (in cells, and
quantised as the optimal rule sees them), the longest route, the arrivals (the end link within ARRIVE_TOL["cfg3"] of
the pick cell), the step of the last arrival, the failed solves, ms of the pairing and of the plan (event-timed) and
ms per control step.
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

K_LIDAR, RAYS = 4, 64
FOLLOW_M = 1.3      # a waypoint counts as reached within this distance [m] (the reference's 1.3)
MODES = ("fixed", "greedy", "optimal")


def run(B=16, T=24, steps=400, seed=0, dev="cuda:0", assign="optimal"):
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import Arrivals, MixedFleetShard, event_ms
    from robot_mpcs_amd.global_planner import GoalAssigner, png_values
    from robot_mpcs_amd.store import STORE as S, BoxerStore, clear_cells, store_map

    if assign not in MODES:
        raise ValueError("assign must be one of " + ", ".join(MODES))
    if not 1 <= B <= T:
        raise ValueError("need 1 <= robots <= goals")
    rng = np.random.default_rng(seed)
    raw = store_map(seed)
    g_raw = torch.from_numpy(png_values(raw)).to(dev)
    g_inf = torch.empty_like(g_raw)
    _lib.grid_inflate_device(g_raw, g_inf, S.cell, S.size_robot, 0.29)
    ok = np.flatnonzero((clear_cells(raw, S.clear_cells) & (g_inf.cpu().numpy() < 0.8)).ravel())
    cells = rng.choice(ok, B + T, replace=False).astype(np.int32)
    starts, goals = cells[:B], cells[B:]
    fleet = BoxerStore(B, seed, dev, K_LIDAR, RAYS, starts, rng)
    d_starts = torch.from_numpy(starts).to(dev)
    ga = GoalAssigner(g_inf, goals)
    paths, lens = ga.plan(d_starts)                       # the optimal pairing, and the cost matrix of all three
    plan_ms = event_ms(lambda: ga.plan(d_starts), 5)
    if assign == "optimal":
        pair_ms = event_ms(lambda: _lib.assign_optimal_device(ga.cost, ga.assignment, ga.scale, ga.total, ga.count,
                                                              ga.steps, ga.work), 5)
        extra = dict(assign_steps=int(ga.steps.item()))
    else:
        if assign == "greedy":
            pair_ms = event_ms(lambda: _lib.assign_greedy_device(ga.cost, ga.assignment), 5)
        else:
            ga.assignment.copy_(torch.arange(B, dtype=torch.int32, device=dev))
            pair_ms = 0.0
        _lib.grid_paths_device(ga.grid, ga.fields, ga.goal_cells, d_starts, ga.assignment, paths, lens, ga.movement,
                               ga.occ, ga.factor)
        lens.masked_fill_(ga.assignment < 0, 0)
        extra = {}
    a = ga.assignment.clamp(min=0).long()
    paired = ga.assignment >= 0
    cost = ga.cost.gather(1, a[:, None])[:, 0]
    paired &= cost < float("inf")
    q = torch.where(paired, torch.round(cost * ga.scale), torch.zeros_like(cost))
    follower = fleet.follower(FOLLOW_M, paths, lens)
    xy = torch.stack([S.x0 + (ga.goal_cells_of() % S.W).double() * S.cell,
                      S.y0 + (ga.goal_cells_of() // S.W).double() * S.cell], 1)
    final = torch.where(paired[:, None], xy, torch.full_like(xy, float("inf")))
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
    ms = 1e3 * (time.perf_counter() - t_loop) / max(steps, 1)

    out = dict(fleet.report(), assign=assign, goals=T, steps=steps, seed=seed, paired=int(paired.sum().item()),
               routes=int((lens > 0).sum().item()),
               route_cost_sum=float(torch.where(paired, cost, torch.zeros_like(cost)).sum().item()),
               route_cost_sum_q=int(q.sum().item()), route_cost_max=float(torch.where(paired, cost, torch.zeros_like(cost)).max().item()),
               route_len_max=int(lens.max().item()), **arrivals.summary(), pairing_ms=round(pair_ms, 4),
               plan_ms=round(plan_ms, 4), ms_per_step=round(ms, 3), arrive_tol_m=tol, **extra)
    fleet.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=16)
    ap.add_argument("--goals", type=int, default=24)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--assign", default="optimal", choices=MODES)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.robots, a.goals, a.steps, a.seed, assign=a.assign)))


if __name__ == "__main__":
    main()
