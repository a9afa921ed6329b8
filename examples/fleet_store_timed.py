#!/usr/bin/env python3
"""Boxers crossing a store on conflict-free timed routes, entirely on the device.  The loop is the one
of examples/fleet_store_lidar.py with the fleet's separating planes beside the lidar planes (``BoxerStore`` with
``neighbours``), run on the same starts and goals in one of two modes:

    plain   plan_batch + RouteFollower: every robot follows its own shortest route, blind to the others' routes
    timed   TimedRoutes + TimedFollower: space-time routes planned for several priority orders at once, the best
            order followed so that no robot passes a cell before the robots planned through it ahead of it

    RouteFollower.step | TimedFollower.step -> LidarPlanes.step -> NeighbourPlanes.step -> solve_scene_device
    -> advance_device(..., exitflag=ef)

Two scenarios: ``store`` draws starts and goals as the other store examples do, pairwise at least three cells apart
among starts and among goals (``pick_spaced_routes``); ``head-on`` puts a robot at each end of four aisles and sends
it to the other end, so that each pair meets head-on in its aisle.

    python examples/fleet_store_timed.py [--robots 16] [--steps 400] [--seed 0] [--scenario store|head-on] [--repair 0]

``--repair R`` has the timed mode repair every priority order on the device for up to R rounds: the robots
that failed or came late are planned first in the next round.

Prints one JSON line per mode: the report fields of the store examples, the arrivals (the end link within
ARRIVE_TOL["cfg3"] of the final goal), the least distance between two end links less r_i + r_j, for the timed mode
the plan's failures, its best order and its last arrival layer, ms per control step and ms of the plan and of one
follower step (event-timed).
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
LAG = 1
T = 128             # the window [layers]: one layer is one cell of travel
ORDERS = 16         # priority orders planned at once
K_LIDAR, K_FLEET, RAYS = 4, 2, 64
FOLLOW_M = 1.3      # a waypoint counts as reached within this distance [m], in both modes (the reference's 1.3)


def head_on_routes(raw, ok, pairs):
    """(starts, goals) of 2 * pairs robots: in each of the first ``pairs`` aisles (the longest run of ``ok`` cells of a
    row, rows at least six apart) one robot at each end of the run, bound for the other end"""
    W = raw.shape[1]
    starts, goals, last = [], [], -10
    for r in range(raw.shape[0]):
        if r - last < 6 or len(starts) == 2 * pairs:
            continue
        row = np.concatenate(([False], ok[r], [False])).astype(np.int8)
        edges = np.flatnonzero(np.diff(row))
        runs = [(int(b - a), int(a), int(b) - 1) for a, b in zip(edges[0::2], edges[1::2])]
        if not runs or max(runs)[0] < 20:
            continue
        _, c0, c1 = max(runs)
        starts += [r * W + c0, r * W + c1]
        goals += [r * W + c1, r * W + c0]
        last = r
    if len(starts) != 2 * pairs:
        raise ValueError("head_on_routes: the store has fewer than %d aisles" % pairs)
    return np.array(starts, np.int32), np.array(goals, np.int32)


def run(B=16, steps=400, seed=0, dev="cuda:0", mode="timed", scenario="store", threshold=None, orders=ORDERS, repair=0):
    import torch
    from robot_mpcs_amd.fleet import Arrivals, MixedFleetShard, event_ms
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.global_planner import (TimedFollower, TimedRoutes, cell_xy, pick_spaced_routes, plan_batch,
                                               png_values)
    from robot_mpcs_amd.store import STORE as S, BoxerStore, clear_cells, store_map

    if mode not in ("plain", "timed"):
        raise ValueError("mode must be plain or timed")
    threshold = FOLLOW_M if threshold is None else float(threshold)
    rng = np.random.default_rng(seed)
    raw = store_map(seed)
    # the planning grid as ``store_routes`` makes it; the routes are the scenario's
    g_raw = torch.from_numpy(png_values(raw)).to(dev)
    g_inf = torch.empty_like(g_raw)
    _lib.grid_inflate_device(g_raw, g_inf, S.cell, S.size_robot, 0.29)
    ok = clear_cells(raw, S.clear_cells) & (g_inf.cpu().numpy() < 0.8)
    if scenario == "store":
        starts, goals = pick_spaced_routes(raw > 0.5, ok, B, rng, S.x0, S.y0, S.cell, SEP2)
    elif scenario == "head-on":
        starts, goals = head_on_routes(raw, ok, B // 2)
    else:
        raise ValueError("scenario must be store or head-on")
    B = len(starts)
    fleet = BoxerStore(B, seed, dev, K_LIDAR, RAYS, starts, rng, neighbours=K_FLEET)
    d_starts, d_goals = torch.from_numpy(starts).to(dev), torch.from_numpy(goals).to(dev)
    extra = {}
    if mode == "plain":
        paths, lens = plan_batch(g_inf, d_starts, d_goals)
        follower = fleet.follower(threshold, paths, lens)
        routes = int((lens > 0).sum().item())
    else:
        tr = TimedRoutes(g_inf, 4, 0.8, T, SEP2, lag=LAG, orders=orders, seed=seed, device=dev, repair=repair)
        paths, status, arrive, best = tr.plan(d_starts, d_goals)
        b = int(best.item())                            # (the one host read of the plan: which order to follow)
        follower = TimedFollower(paths[b].contiguous(), S.W, S.x0, S.y0, S.cell, threshold, SEP2, LAG)
        st, ar = status[b].cpu().numpy(), arrive[b].cpu().numpy()
        routes = int((st == 0).sum())
        extra = dict(best_order=b, plan_failures=int((st > 0).sum()), plan_late=int((ar > T).sum()),
                     plan_last_arrival_layer=int(ar.max()), plan_failures_by_order=(status > 0).sum(dim=1).cpu().tolist(),
                     plan_ms=round(event_ms(lambda: tr.plan(d_starts, d_goals), 5), 4))
        if repair:
            extra.update(repair=repair, rounds_run=tr.rounds_run.cpu().tolist(), round_best=tr.round_best.cpu().tolist())
    final = torch.from_numpy(cell_xy(goals, S.W, S.x0, S.y0, S.cell)).to(dev)
    tol = MixedFleetShard.ARRIVE_TOL["cfg3"]
    arrivals = Arrivals(B, dev)
    upper = torch.triu(torch.ones((B, B), dtype=torch.bool, device=dev), diagonal=1)
    rsum = fleet.rad[:, None] + fleet.rad[None, :]
    min_gap = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    waits = torch.zeros((), dtype=torch.int64, device=dev)

    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    for step in range(steps):
        follower.step(fleet.x, fleet.goal)
        if mode == "timed":
            waits += (follower.blocked >= 0).sum()
        fleet.scan()
        ee = fleet.drive()
        d = (ee[:, None, :] - ee[None, :, :]).norm(dim=2)
        min_gap = torch.minimum(min_gap, torch.where(upper, d - rsum, torch.full_like(d, float("inf"))).min())
        arrivals.update((ee - final).norm(dim=1) < tol, step)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / steps

    follow_ms = event_ms(lambda: follower.step(fleet.x, fleet.goal), 20)
    out = dict(fleet.report(), mode=mode, scenario=scenario, steps=steps, seed=seed, K_fleet=K_FLEET, threshold_m=threshold,
               routes=routes, **arrivals.summary(), min_pair_gap_m=float(min_gap.item()), robot_steps_waited=int(waits.item()),
               ms_per_step=round(ms, 3), follower_step_ms=round(follow_ms, 4), arrive_tol_m=tol, **extra)
    fleet.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=16)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--scenario", default="store")
    ap.add_argument("--repair", type=int, default=0, help="rounds of order repair on the device (DESIGN.md 27)")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    for mode in ("plain", "timed"):
        print(json.dumps(run(a.robots, a.steps, a.seed, mode=mode, scenario=a.scenario, repair=a.repair)))


if __name__ == "__main__":
    main()
