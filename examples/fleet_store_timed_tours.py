#!/usr/bin/env python3
"""More picks than boxers in a store on conflict-free timed tours, entirely on the device.  The loop is
the one of examples/fleet_store_timed.py -- the fleet's separating planes beside the lidar planes (``BoxerStore`` with
``neighbours``) -- with 16 boxers, 24 pick cells and at most K = 2 picks per robot, run on the same starts and picks in
one of two plans:

    static  TourPlanner.plan + TourFollower: every robot descends the fields of its picks, blind to the
            others' routes
    timed   TimedTours + TimedTourFollower: the same tours planned in space-time for several priority orders at once,
            with ``dwell`` layers on every pick; the best order is followed so that no robot passes a cell before the
            robots planned through it ahead of it, and a pick is served only when the end link is on it

    TourFollower.step | TimedTourFollower.step -> LidarPlanes.step -> NeighbourPlanes.step -> solve_scene_device
    -> advance_device(..., exitflag=ef)

    python examples/fleet_store_timed_tours.py [--robots 16] [--goals 24] [--K 2] [--steps 400] [--seed 0]
                                               [--plan timed|static] [--dwell 3] [--park last|start]

Both followers are handed the end links' positions: a pick counts as served when the end link is within
ARRIVE_TOL["cfg3"] of its cell.  The loop ends once every planned pick is served and, in the timed plan, stood on for
``dwell`` steps.  Prints one JSON line: the report fields of the store examples, the picks planned and served, the step
of the last service, the failed solves, the least distance between two end links less r_i + r_j and its step, the
fewest consecutive steps a robot stood on a pick, and ms of the plan (event-timed).
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

SEP2 = 9            # three cells = 1.35 m >= 2 r_body between two robots' cells within LAG layers
START_SEP2 = 25     # five cells = 2.25 m >= 2 r_body + 2 ee_offset between two starts: the end links, 0.4 m ahead of
                    # the base cells under headings drawn at random, are clear of each other at step 0
LAG = 1
T = 255             # the window [layers]: two legs and their dwell
ORDERS = 16         # priority orders planned at once
K_LIDAR, K_FLEET, RAYS = 4, 2, 64
FOLLOW_M = 1.3      # a waypoint that is no stop counts as reached within this distance [m] (the reference's 1.3)
PLANS = ("timed", "static")


def run(B=16, picks=24, K=2, steps=400, seed=0, dev="cuda:0", plan="timed", dwell=3, park="last", orders=ORDERS,
        check_every=4, threshold=FOLLOW_M):
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import MixedFleetShard, event_ms
    from robot_mpcs_amd.global_planner import (TimedTourFollower, TimedTours, TourFollower, TourPlanner, cell_xy,
                                               pick_spaced_tours, png_values)
    from robot_mpcs_amd.store import STORE as S, BoxerStore, clear_cells, store_map

    if plan not in PLANS:
        raise ValueError("plan must be one of " + ", ".join(PLANS))
    if not 1 <= B <= picks <= B * K:
        raise ValueError("need 1 <= robots <= goals <= robots * K")
    rng = np.random.default_rng(seed)
    raw = store_map(seed)
    g_raw = torch.from_numpy(png_values(raw)).to(dev)
    g_inf = torch.empty_like(g_raw)
    _lib.grid_inflate_device(g_raw, g_inf, S.cell, S.size_robot, 0.29)
    ok = clear_cells(raw, S.clear_cells) & (g_inf.cpu().numpy() < 0.8)
    starts, goals = pick_spaced_tours(raw > 0.5, ok, B, picks, rng, S.x0, S.y0, S.cell, SEP2, START_SEP2)
    fleet = BoxerStore(B, seed, dev, K_LIDAR, RAYS, starts, rng, neighbours=K_FLEET)
    d_starts = torch.from_numpy(starts).to(dev)
    tol = MixedFleetShard.ARRIVE_TOL["cfg3"]
    planner = TourPlanner(g_inf, goals, K)
    extra = {}
    if plan == "static":
        paths, lens, stop_at = planner.plan(d_starts)
        plan_ms = event_ms(lambda: planner.plan(d_starts), 5)
        follower = TourFollower(paths, lens, stop_at, S.W, S.x0, S.y0, S.cell, threshold=threshold, stop_tol=tol)
        planned_at = stop_at >= 0
    else:
        tt = TimedTours(planner, T, SEP2, lag=LAG, dwell=dwell, orders=orders, park=park, seed=seed)
        paths, serve_at, status, served, arrive, best = tt.plan(d_starts)
        b = int(best.item())                            # (the one host read of the plan: which order to follow)
        plan_ms = event_ms(lambda: tt.plan(d_starts), 5)
        follower = TimedTourFollower(paths[b], serve_at[b], S.W, S.x0, S.y0, S.cell, threshold, tol, SEP2, LAG)
        planned_at = serve_at[b] >= 0
        st = status[b].cpu().numpy()
        extra = dict(best_order=b, plan_failures=int((st > 0).sum()), plan_unserved=int(tt.unserved[b].item()),
                     plan_unserved_by_order=tt.unserved.cpu().tolist(), plan_last_service_layer=int(serve_at[b].max().item()),
                     plan_last_arrival_layer=int(arrive[b].max().item()), dwell=dwell, park=park)
    planned = int(planned_at.sum().item())
    # the centres of every robot's picks, and how long it has stood on each without a break
    tours = planner.tours.clamp(min=0).long()
    pick_xy = torch.from_numpy(cell_xy(goals, S.W, S.x0, S.y0, S.cell)).to(dev)[tours]            # (B, K, 2)
    stood = torch.zeros((B, K), dtype=torch.int64, device=dev)
    stood_max = torch.zeros((B, K), dtype=torch.int64, device=dev)
    upper = torch.triu(torch.ones((B, B), dtype=torch.bool, device=dev), diagonal=1)
    rsum = fleet.rad[:, None] + fleet.rad[None, :]
    min_gap = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    gap_step = torch.zeros((), dtype=torch.int64, device=dev)
    x = fleet.x
    ee = x[:, :2] + S.ee_offset * torch.stack([torch.cos(x[:, 2]), torch.sin(x[:, 2])], 1)
    need = dwell if plan == "timed" else 0

    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    done = 0
    for step in range(steps):
        follower.step(ee, fleet.goal)
        fleet.scan()
        ee = fleet.drive()
        d = (ee[:, None, :] - ee[None, :, :]).norm(dim=2)
        gap = torch.where(upper, d - rsum, torch.full_like(d, float("inf"))).min()
        gap_step = torch.where(gap < min_gap, torch.full_like(gap_step, step), gap_step)
        min_gap = torch.minimum(min_gap, gap)
        on = (ee[:, None, :] - pick_xy).norm(dim=2) <= tol
        stood = (stood + 1) * on
        stood_max = torch.maximum(stood_max, stood)
        done = step + 1
        if check_every and done % check_every == 0 and int(follower.served_count().item()) == planned and \
                bool((stood_max[planned_at] >= need).all().item()):
            break
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / max(done, 1)

    served = follower.served
    out = dict(fleet.report(), plan=plan, goals=picks, tour_K=K, steps=done, seed=seed, K_fleet=K_FLEET,
               picks_planned=planned, picks_served=int((served >= 0).sum().item()),
               last_service_step=int(served.max().item()) + 1, min_pair_gap_m=float(min_gap.item()),
               min_pair_gap_step=int(gap_step.item()),
               min_steps_on_a_pick=int(stood_max[planned_at].min().item()) if planned else 0,
               plan_ms=round(plan_ms, 4), ms_per_step=round(ms, 3), stop_tol_m=tol, **extra)
    fleet.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=16)
    ap.add_argument("--goals", type=int, default=24)
    ap.add_argument("--K", type=int, default=2)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--plan", default="timed", choices=PLANS)
    ap.add_argument("--dwell", type=int, default=3)
    ap.add_argument("--park", default="last", choices=("last", "start"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.robots, a.goals, a.K, a.steps, a.seed, plan=a.plan, dwell=a.dwell, park=a.park)))


if __name__ == "__main__":
    main()
