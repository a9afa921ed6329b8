#!/usr/bin/env python3
"""More picks than boxers in a store, entirely on the device: every robot gets a tour of up to K pick
cells and stops at each of them, then the loop of examples/fleet_store_dispatch.py drives the routes.  B boxers and T
pick cells on random clear cells, drawn as the dispatch example draws them, B <= T <= B K, and one of three plans:

    tours-span  TourPlanner, mode "span": rmpc_tours_device with the longest tour as short as the rule gets it
    tours-sum   TourPlanner, mode "sum": the least sum of the tours
    rounds      what GoalAssigner alone can do: K rounds of the minimum-cost assignment, round r from the cells the
                robots reached in round r - 1 to the picks that are left

    TourFollower.step -> LidarPlanes.step -> solve_scene_device -> advance_device(..., exitflag=ef)

    python examples/fleet_store_tours.py [--robots 16] [--goals 24] [--K 2] [--steps 400] [--seed 0]
                                         [--plan tours-span|tours-sum|rounds]

The follower is handed the end links' positions, since a pick counts as served when the end link is within
ARRIVE_TOL["cfg3"] of its cell.  The loop ends once every planned pick is served.  Prints one JSON line: the report fields
of the store examples, the picks planned and served, the step of the last service, the sum and the span of the quantised
tour costs, the failed solves, the least distance between two end links (reported, not gated: these robots do not see
each other, as in the dispatch example), ms of the plan (event-timed) and ms per control step.
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
FOLLOW_M = 1.3      # a waypoint that is no stop counts as reached within this distance [m] (the reference's 1.3)
PLANS = ("tours-span", "tours-sum", "rounds")


class RoundsPlanner:
    """K rounds of ``GoalAssigner``'s assignment on the fields of all picks: round r pairs the robots, from the cells
    they reached in round r - 1, with the picks nobody has taken.  A robot left without a pick in one round takes none
    later.  The same outputs as ``TourPlanner.plan``, and the quantised cost of every robot's legs."""

    def __init__(self, grid, goal_cells, K, B, scale=1024.0):
        import torch
        from robot_mpcs_amd.global_planner import GoalAssigner
        self.ga, self.K, self.B = GoalAssigner(grid, goal_cells, scale=scale), K, B
        dev, T, max_len = self.ga.grid.device, self.ga.T, self.ga.max_len
        self.ga._sized(B)
        self.tours = torch.empty((B, K), dtype=torch.int32, device=dev)
        self.legs = torch.zeros((K, B, max_len), dtype=torch.int32, device=dev)
        self.leg_lens = torch.zeros((K, B), dtype=torch.int32, device=dev)
        self.paths = torch.zeros((B, K * max_len), dtype=torch.int32, device=dev)
        self.tour_cost = torch.zeros(B, dtype=torch.int64, device=dev)
        self.T = T

    def plan(self, start_cells):
        import torch
        from robot_mpcs_amd import _lib
        from robot_mpcs_amd.global_planner.tours import join_legs
        ga = self.ga
        at = start_cells
        taken = torch.zeros(self.T, dtype=torch.bool, device=at.device)
        active = torch.ones(self.B, dtype=torch.bool, device=at.device)
        self.tour_cost.zero_()
        for k in range(self.K):
            _lib.grid_route_costs_device(ga.grid, ga.fields, at, ga.cost, ga.movement, ga.occ, ga.factor)
            ga.cost.masked_fill_(taken[None, :] | ~active[:, None], float("inf"))
            _lib.assign_optimal_device(ga.cost, ga.assignment, ga.scale, ga.total, ga.count, ga.steps, ga.work)
            a = ga.assignment
            active = active & (a >= 0)
            self.tours[:, k] = a
            hit = torch.zeros(self.T + 1, dtype=torch.bool, device=at.device)
            hit[torch.where(a >= 0, a, torch.full_like(a, self.T)).long()] = True
            taken = taken | hit[:self.T]
            q = torch.round(ga.cost.gather(1, a.clamp(min=0).long()[:, None])[:, 0] * ga.scale)
            self.tour_cost += torch.where(a >= 0, q, torch.zeros_like(q)).long()
            _lib.grid_paths_device(ga.grid, ga.fields, ga.goal_cells, at, a, self.legs[k], self.leg_lens[k], ga.movement,
                                   ga.occ, ga.factor)
            at = torch.where(a >= 0, ga.goal_cells[a.clamp(min=0).long()], at).contiguous()
        self.lens, self.stop_at = join_legs(self.legs, self.leg_lens, self.paths)
        return self.paths, self.lens, self.stop_at


def run(B=16, T=24, K=2, steps=400, seed=0, dev="cuda:0", plan="tours-span", check_every=4):
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import MixedFleetShard, event_ms
    from robot_mpcs_amd.global_planner import TourFollower, TourPlanner, png_values
    from robot_mpcs_amd.store import STORE as S, BoxerStore, clear_cells, store_map

    if plan not in PLANS:
        raise ValueError("plan must be one of " + ", ".join(PLANS))
    if not 1 <= B <= T <= B * K:
        raise ValueError("need 1 <= robots <= goals <= robots * K")
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
    if plan == "rounds":
        planner = RoundsPlanner(g_inf, goals, K, B)
        extra = {}
    else:
        planner = TourPlanner(g_inf, goals, K, mode=plan.split("-")[1])
    paths, lens, stop_at = planner.plan(d_starts)
    plan_ms = event_ms(lambda: planner.plan(d_starts), 5)
    if plan != "rounds":
        extra = dict(build_steps=int(planner.build_steps.item()), rounds=int(planner.rounds.item()))
    planned = int((stop_at >= 0).sum().item())
    tol = MixedFleetShard.ARRIVE_TOL["cfg3"]
    follower = TourFollower(paths, lens, stop_at, S.W, S.x0, S.y0, S.cell, threshold=FOLLOW_M, stop_tol=tol)
    x = fleet.x
    ee = x[:, :2] + S.ee_offset * torch.stack([torch.cos(x[:, 2]), torch.sin(x[:, 2])], 1)
    apart = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    far = torch.eye(B, dtype=torch.float64, device=dev) * 1e9

    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    done = 0
    for step in range(steps):
        follower.step(ee, fleet.goal)
        fleet.scan()
        ee = fleet.drive()
        apart = torch.minimum(apart, (torch.cdist(ee, ee) + far).min())
        done = step + 1
        if check_every and done % check_every == 0 and int(follower.served_count().item()) == planned:
            break
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / max(done, 1)

    served = follower.served
    out = dict(fleet.report(), plan=plan, goals=T, tour_K=K, steps=done, seed=seed, picks_planned=planned,
               picks_served=int((served >= 0).sum().item()), last_service_step=int(served.max().item()) + 1,
               tour_cost_sum_q=int(planner.tour_cost.sum().item()), tour_cost_span_q=int(planner.tour_cost.max().item()),
               route_len_max=int(lens.max().item()), min_pair_distance_m=float(apart.item()), plan_ms=round(plan_ms, 4),
               ms_per_step=round(ms, 3), stop_tol_m=tol, **extra)
    fleet.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=16)
    ap.add_argument("--goals", type=int, default=24)
    ap.add_argument("--K", type=int, default=2)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--plan", default="tours-span", choices=PLANS)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.robots, a.goals, a.K, a.steps, a.seed, plan=a.plan)))


if __name__ == "__main__":
    main()
