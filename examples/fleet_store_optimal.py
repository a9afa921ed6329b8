#!/usr/bin/env python3
"""Boxers crossing a store on optimal timed routes, entirely on the device.  The loop is the one of
examples/fleet_store_timed.py; the plan is ``OptimalTimedRoutes``: conflict-based search over the same cells, layers and
conflicts, which either proves the least sum of arrivals or leaves a lower bound on it.  Beside it the best repaired
prioritised plan (``TimedRoutes`` with ``repair``) is made from the same starts and goals, and its sum of arrivals is held
against the search's cost and bound.

    OptimalTimedRoutes.plan -> TimedFollower.step -> LidarPlanes.step -> NeighbourPlanes.step -> solve_scene_device
    -> advance_device(..., exitflag=ef)

The fleet follows the search's plan when the search reports a conflict-free node, the prioritised plan otherwise.

    python examples/fleet_store_optimal.py [--robots 2] [--steps 300] [--seed 0]

On store seed 0 under the class defaults (nodes 4096, expand 16, rounds 64) the restatement of tests/cbs_reference.py
proves the optimum for 2 robots (cost 85) and for none of 4, 8 and 16: there the search ends ROUNDS with the root's
bound (173, 316, 637), the store's open aisles being the plateau of equal-cost routes on which plain conflict-based
search is known to stall.  ``ROBOTS`` is therefore 2; larger fleets are run for their bound.

Prints one JSON line: the report fields of the store examples, outcome, cost, bound, created, expanded and rounds_run of
the search, ``prioritised_sum`` (None when every order has a failure), which plan was followed, the arrivals and the
least distance between two end links less r_i + r_j.
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
ROBOTS = 2                    # the largest fleet the search proves optimal on store seed 0 under the class defaults


def run(B=ROBOTS, steps=300, seed=0, dev="cuda:0", rounds=None):
    import torch
    from robot_mpcs_amd.fleet import Arrivals, MixedFleetShard, event_ms
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.global_planner import (OptimalTimedRoutes, TimedFollower, TimedRoutes, cell_xy, pick_spaced_routes,
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

    kw = {} if rounds is None else dict(rounds=rounds)
    otr = OptimalTimedRoutes(g_inf, 4, 0.8, T, SEP2, lag=LAG, device=dev, **kw)
    paths, status, arrive, info = otr.plan(d_starts, d_goals)
    tr = TimedRoutes(g_inf, 4, 0.8, T, SEP2, lag=LAG, orders=ORDERS, seed=seed, device=dev, repair=REPAIR)
    t_paths, t_status, t_arrive, t_best = tr.plan(d_starts, d_goals)
    gap = otr.gap(t_arrive[t_best.clamp(min=0)[0].long()])
    # the host reads of the plans: what the search found and which order to fall back on
    found = dict(zip((n.lower() for n in _lib.CBS_INFO_NAMES), info.cpu().tolist()))
    b = int(t_best.item())
    clean = b >= 0 and bool((t_status[b] <= 0).all().item())
    optimal = bool(found["conflict_free"])
    follower = TimedFollower((paths if optimal else t_paths[b]).contiguous(), S.W, S.x0, S.y0, S.cell, FOLLOW_M, SEP2, LAG)
    plan_ms = event_ms(lambda: otr.plan(d_starts, d_goals), 3)

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
    out = dict(fleet.report(), steps=steps, seed=seed, **found, followed="optimal" if optimal else "prioritised",
               prioritised_sum=int(t_arrive[b].sum().item()) if clean else None,
               prioritised_less_bound=int(gap[0].item()) if clean else None, **arrivals.summary(),
               min_pair_gap_m=float(min_gap.item()), plan_ms=round(plan_ms, 3), arrive_tol_m=tol)
    fleet.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=ROBOTS)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=None, help="rounds of the search (the class default otherwise)")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.robots, a.steps, a.seed, rounds=a.rounds)))


if __name__ == "__main__":
    main()
