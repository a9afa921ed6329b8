#!/usr/bin/env python3
"""Boxers crossing a store on traffic-aware routes, entirely on the device.  The store crossing of
examples/fleet_store_timed.py -- the same map, starts, goals, lidar planes and separating planes, seed 0 -- with the
fleet following, through ``RouteFollower``, one of two kinds of routes:

    plain     plan_batch: every robot's own shortest route, blind to the others' routes
    traffic   TrafficRoutes: routes that pay for the cells other routes use and for steps against their direction,
              re-planned one robot at a time (``--groups 0``: as many groups as robots) for ``--rounds`` rounds

    RouteFollower.step -> LidarPlanes.step -> NeighbourPlanes.step -> solve_scene_device -> advance_device(..., exitflag=ef)

    python examples/fleet_store_traffic.py [--robots 16] [--steps 400] [--seed 0] [--groups 0] [--rounds 4]

Prints one JSON line per mode: the report fields of the store examples (failed solves among them), the arrivals (the end
link within ARRIVE_TOL["cfg3"] of the final goal), the least distance between two end links less r_i + r_j, the score
(L, V, C) of the routes' flow table -- one row for the plain routes, one per round for the traffic-aware ones --, ms per
control step and, for the traffic mode, ms of ``TrafficRoutes.plan`` (event-timed).
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

SEP2 = 9            # starts, and goals, pairwise at least three cells apart, as in fleet_store_timed.py
K_LIDAR, K_FLEET, RAYS = 4, 2, 64
FOLLOW_M = 1.3      # a waypoint counts as reached within this distance [m] (the reference's 1.3)


def run(B=16, steps=400, seed=0, dev="cuda:0", mode="traffic", groups=0, rounds=4, costs=None, threshold=None, keep=None):
    """``keep``: a dict that receives the planning grid, the starts, the goals and the routes followed (numpy)."""
    import torch
    from robot_mpcs_amd.fleet import Arrivals, MixedFleetShard, event_ms
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.global_planner import TrafficRoutes, cell_xy, pick_spaced_routes, plan_batch, png_values
    from robot_mpcs_amd.store import STORE as S, BoxerStore, clear_cells, store_map

    if mode not in ("plain", "traffic"):
        raise ValueError("mode must be plain or traffic")
    threshold = FOLLOW_M if threshold is None else float(threshold)
    rng = np.random.default_rng(seed)
    raw = store_map(seed)
    g_raw = torch.from_numpy(png_values(raw)).to(dev)
    g_inf = torch.empty_like(g_raw)
    _lib.grid_inflate_device(g_raw, g_inf, S.cell, S.size_robot, 0.29)
    ok = clear_cells(raw, S.clear_cells) & (g_inf.cpu().numpy() < 0.8)
    starts, goals = pick_spaced_routes(raw > 0.5, ok, B, rng, S.x0, S.y0, S.cell, SEP2)
    B = len(starts)
    fleet = BoxerStore(B, seed, dev, K_LIDAR, RAYS, starts, rng, neighbours=K_FLEET)
    d_starts, d_goals = torch.from_numpy(starts).to(dev), torch.from_numpy(goals).to(dev)
    costs = costs if costs is not None else _lib.traffic_costs()
    extra = {}
    if mode == "plain":
        paths, lens = plan_batch(g_inf, d_starts, d_goals)
        flow = torch.zeros((_lib.TRAFFIC_PLANES, S.H, S.W), dtype=torch.int32, device=dev)
        score = torch.zeros(3, dtype=torch.int64, device=dev)
        _lib.grid_traffic_add_device(flow, paths, lens)
        _lib.grid_traffic_score_device(flow, score, costs.base_axial, costs.base_diag)
        scores = [score.cpu().tolist()]
    else:
        groups = groups or B
        tr = TrafficRoutes(g_inf, d_starts, d_goals, costs=costs, groups=groups, rounds=rounds)
        tr.plan()
        paths, lens = tr.paths.clone(), tr.lens.clone()      # (the follower's own: the timing below plans again)
        scores = tr.scores.cpu().tolist()
        extra = dict(groups=groups, rounds=rounds, plan_ms=round(event_ms(tr.plan, 5), 4))
    follower = fleet.follower(threshold, paths, lens)
    routes = int((lens > 0).sum().item())
    if keep is not None:
        keep.update(grid=g_inf.cpu().numpy(), starts=starts, goals=goals, paths=paths.cpu().numpy(), lens=lens.cpu().numpy())
    final = torch.from_numpy(cell_xy(goals, S.W, S.x0, S.y0, S.cell)).to(dev)
    tol = MixedFleetShard.ARRIVE_TOL["cfg3"]
    arrivals = Arrivals(B, dev)
    upper = torch.triu(torch.ones((B, B), dtype=torch.bool, device=dev), diagonal=1)
    rsum = fleet.rad[:, None] + fleet.rad[None, :]
    min_gap = torch.full((), float("inf"), dtype=torch.float64, device=dev)

    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    for step in range(steps):
        follower.step(fleet.x, fleet.goal)
        fleet.scan()
        ee = fleet.drive()
        d = (ee[:, None, :] - ee[None, :, :]).norm(dim=2)
        min_gap = torch.minimum(min_gap, torch.where(upper, d - rsum, torch.full_like(d, float("inf"))).min())
        arrivals.update((ee - final).norm(dim=1) < tol, step)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / steps

    out = dict(fleet.report(), mode=mode, steps=steps, seed=seed, K_fleet=K_FLEET, threshold_m=threshold, routes=routes,
               **arrivals.summary(), min_pair_gap_m=float(min_gap.item()), scores_LVC=scores, ms_per_step=round(ms, 3),
               arrive_tol_m=tol, **extra)
    fleet.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=16)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--groups", type=int, default=0, help="0: one robot per group")
    ap.add_argument("--rounds", type=int, default=4)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    for mode in ("plain", "traffic"):
        print(json.dumps(run(a.robots, a.steps, a.seed, mode=mode, groups=a.groups, rounds=a.rounds)))


if __name__ == "__main__":
    main()
