#!/usr/bin/env python3
"""Sixteen boxers crossing a store on a searched plan with a proven quality, entirely on the device.  The
loop is the one of examples/fleet_store_timed.py; the plan is ``BoundedTimedRoutes``: focal conflict-based search over
the same cells, layers and conflicts, which ends with a conflict-free plan for the whole fleet and a lower bound, the
plan's sum of arrivals within the factor ``w`` of it.  Beside it the best repaired prioritised plan (``TimedRoutes`` with
``repair``) is made from the same starts and goals, and its sum of arrivals is reported next to the search's cost and
bound.

    BoundedTimedRoutes.plan -> TimedFollower.step -> LidarPlanes.step -> NeighbourPlanes.step -> solve_scene_device
    -> advance_device(..., exitflag=ef)

The fleet follows the search's plan when the search reports a conflict-free node, the prioritised plan otherwise.

    python examples/fleet_store_bounded.py [--robots 16] [--steps 300] [--seed 0] [--w 11 10]

On store seed 0 at w = 11/10, one node per round, the restatement of tests/ecbs_reference.py is through after 351
expansions: cost 696 over the bound 633, where the best of 16 repaired orders sums to 736 and plain conflict-based search
is still at the root's bound after 975 expansions (examples/fleet_store_optimal.py).

Prints one JSON line: the report fields of the store examples, the search's info by name, ``ratio`` = cost / bound,
``prioritised_sum`` (None when every order has a failure), which plan was followed, the arrivals and the least distance
between two end links less r_i + r_j.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEP2, LAG, T = 9, 1, 128      # those of examples/fleet_store_timed.py
ORDERS, REPAIR = 16, 3        # the prioritised plan beside it: the best of 16 orders, 3 repair rounds
K_LIDAR, K_FLEET, RAYS = 4, 2, 64
FOLLOW_M = 1.3
ROBOTS = 16
W = (11, 10)
NODES, ROUNDS = 2048, 512     # 351 expansions on store seed 0 (tests/ecbs_cases.py), with room for other seeds


def run(B=ROBOTS, steps=300, seed=0, dev="cuda:0", w=W, rounds=ROUNDS, nodes=NODES):
    import torch
    from robot_mpcs_amd.fleet import Arrivals, MixedFleetShard, event_ms
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.global_planner import (BoundedTimedRoutes, TimedFollower, TimedRoutes, cell_xy, pick_spaced_routes,
                                               png_values)
    from robot_mpcs_amd.store import STORE as S, BoxerStore, clear_cells, store_map

    rng = np.random.default_rng(seed)
    raw = store_map(seed)
    g_raw = torch.from_numpy(png_values(raw)).to(dev)
    g_inf = torch.empty_like(g_raw)
    _lib.grid_inflate_device(g_raw, g_inf, S.cell, S.size_robot, 0.29)
    ok = clear_cells(raw, S.clear_cells) & (g_inf.cpu().numpy() < 0.8)
    starts, goals = pick_spaced_routes(raw > 0.5, ok, B, rng, S.x0, S.y0, S.cell, SEP2)
    fleet = BoxerStore(B, seed, dev, K_LIDAR, RAYS, starts, rng, neighbours=K_FLEET)
    d_starts, d_goals = torch.from_numpy(starts).to(dev), torch.from_numpy(goals).to(dev)

    btr = BoundedTimedRoutes(g_inf, 4, 0.8, T, SEP2, w=w, lag=LAG, nodes=nodes, expand=1, rounds=rounds, device=dev)
    paths, status, arrive, info = btr.plan(d_starts, d_goals)
    tr = TimedRoutes(g_inf, 4, 0.8, T, SEP2, lag=LAG, orders=ORDERS, seed=seed, device=dev, repair=REPAIR)
    t_paths, t_status, t_arrive, t_best = tr.plan(d_starts, d_goals)
    gap = btr.gap(t_arrive[t_best.clamp(min=0)[0].long()])
    ratio = btr.ratio()
    # the host reads of the plans: what the search found and which order to fall back on
    found = dict(zip((n.lower() for n in _lib.ECBS_INFO_NAMES), info.cpu().tolist()))
    cost, bound = ratio.cpu().tolist()
    b = int(t_best.item())
    clean = b >= 0 and bool((t_status[b] <= 0).all().item())
    searched = bool(found["conflict_free"])
    follower = TimedFollower((paths if searched else t_paths[b]).contiguous(), S.W, S.x0, S.y0, S.cell, FOLLOW_M, SEP2, LAG)
    plan_ms = event_ms(lambda: btr.plan(d_starts, d_goals), 3)

    final = torch.from_numpy(cell_xy(goals, S.W, S.x0, S.y0, S.cell)).to(dev)
    tol = MixedFleetShard.ARRIVE_TOL["cfg3"]
    arrivals = Arrivals(B, dev)
    upper = torch.triu(torch.ones((B, B), dtype=torch.bool, device=dev), diagonal=1)
    rsum = fleet.rad[:, None] + fleet.rad[None, :]
    min_gap = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    for step in range(steps):
        follower.step(fleet.x, fleet.goal)
        fleet.scan()
        ee = fleet.drive()
        d = (ee[:, None, :] - ee[None, :, :]).norm(dim=2)
        min_gap = torch.minimum(min_gap, torch.where(upper, d - rsum, torch.full_like(d, float("inf"))).min())
        arrivals.update((ee - final).norm(dim=1) < tol, step)
    torch.cuda.synchronize()
    out = dict(fleet.report(), steps=steps, seed=seed, w=list(w), **found,
               ratio=round(cost / bound, 4) if searched and bound > 0 else None,
               followed="searched" if searched else "prioritised",
               prioritised_sum=int(t_arrive[b].sum().item()) if clean else None,
               prioritised_less_cost=int(gap[1].item()) if clean and searched else None, **arrivals.summary(),
               min_pair_gap_m=float(min_gap.item()), plan_ms=round(plan_ms, 3), arrive_tol_m=tol)
    fleet.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=ROBOTS)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--w", type=int, nargs=2, default=list(W), metavar=("NUM", "DEN"))
    ap.add_argument("--rounds", type=int, default=ROUNDS, help="rounds of the search, one node each")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.robots, a.steps, a.seed, w=tuple(a.w), rounds=a.rounds)))


if __name__ == "__main__":
    main()
