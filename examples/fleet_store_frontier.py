#!/usr/bin/env python3
"""Boxers exploring a store nobody has mapped, without goals: frontier exploration on the device.  The store, the
constants, the boxer model and ``LidarPlanes`` are those of examples/fleet_store_lidar.py; the robots start packed into
one corner (``corner_starts``: the cells nearest it that are free on the map dilated by two cells) and nobody hands
them a goal.  Every control step, all on one stream:

    RouteFollower.step -> LidarPlanes.step -> FleetMap.mark -> solve_scene_device -> advance_device(..., exitflag=ef)

and at step 0 and every ``--replan-every`` steps, after the mark:

    FrontierGoals.replan -> frontier_cells()

``FrontierGoals.replan`` (robot_mpcs_amd/utils/exploration.py) classifies the evidence, enlarges the map, finds the
frontier -- the known free cells next to unknown space --, builds one cost-to-go field to the nearest frontier cell
and gives every robot the route down that field.  ``frontier_cells()`` is the loop's one host read: the run ends at the
first re-plan that finds no frontier, or after ``--steps`` control steps.

    python examples/fleet_store_frontier.py [--robots 64] [--steps 3000] [--seed 0] [--replan-every 10]

Prints one JSON line: the step at which exploration ended (null if it did not), the store's free cells and those seen,
the seen cells and those among them classified against the true map, failed robot-steps, the least distance from the
end link and from the base centre to any shelf box, ms per control step and ms of ``FrontierGoals.replan`` (median of
20 event-timed calls).
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import fleet_store_lidar as store  # noqa: E402  (the store, its constants and helpers)


def run(B=64, steps=3000, seed=0, dev="cuda:0", K=4, rays=64, threshold=1.3, replan_every=10):
    import torch
    from robot_mpcs_amd.fleet import dev_f64, event_ms, limit_tensors, make_block, step_block
    from robot_mpcs_amd.global_planner import RouteFollower, cell_xy, shelf_map
    from robot_mpcs_amd.scenarios import LIMITS, make_scenario
    from robot_mpcs_amd.utils.exploration import FrontierGoals, corner_starts
    from robot_mpcs_amd.utils.lidar import LidarPlanes, boxes_from_grid
    from robot_mpcs_amd.utils.mapping import FleetMap

    H, W, CELL, X0, Y0 = store.H, store.W, store.CELL, store.X0, store.Y0
    rng = np.random.default_rng(seed)
    raw = shelf_map(H, W, seed=seed, aisle=store.AISLE, gap=store.GAP, shelf=store.SHELF)
    starts = corner_starts(raw, B, store.CLEAR_CELLS)
    boxes_np = boxes_from_grid(raw, X0, Y0, CELL)
    boxes = dev_f64(boxes_np, dev)

    sc = make_scenario("boxer", B=B, seed=seed, number_obstacles=K)
    xinit = np.zeros((B, sc.desc["nx"]))
    xinit[:, :2] = cell_xy(starts, W, X0, Y0, CELL)
    xinit[:, 2] = rng.uniform(-math.pi, math.pi, B)
    lp = LidarPlanes(B, sc.desc["N"], K, boxes=boxes_np, rays=rays, offset=(store.EE_OFFSET, 0.0), device=dev)
    goal = dev_f64(np.concatenate([xinit[:, :2], np.zeros((B, 1))], 1), dev)
    f = make_block(sc.desc, sc.setup["mpc"]["weights"], B, xinit, dev, goal=goal,
                   r_body=dev_f64(np.full(B, store.R_BODY), dev), lin_constrs=lp.planes,
                   **limit_tensors(*LIMITS["boxer"], B, dev))
    tx, z, ef = f["x"], f["z"], f["ef"]

    fmap = FleetMap(B, H, W, X0, Y0, CELL, rays, lp.max_range, lp.offset, lp.height, device=dev)
    fg = FrontierGoals(fmap, store.SIZE_ROBOT, 0.29)
    follower = RouteFollower(torch.zeros((B, fg.max_len), dtype=torch.int32, device=dev),
                             torch.zeros(B, dtype=torch.int32, device=dev), W, X0, Y0, CELL, threshold=threshold)

    fails = torch.zeros((), dtype=torch.int64, device=dev)
    ee_clear = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    base_clear = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    ended, replans, frontier, done = None, 0, None, 0

    def ee_of(x):
        return x[:, :2] + store.EE_OFFSET * torch.stack([torch.cos(x[:, 2]), torch.sin(x[:, 2])], 1)

    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    for step in range(steps):
        follower.step(tx, goal)
        lp.step(tx, z if step > 0 else None, ef if step > 0 else None)
        fmap.mark(tx, lp.points, lp.ranges)
        if step % replan_every == 0:
            fg.replan(follower, tx)
            replans += 1
            frontier = fg.frontier_cells()
            if frontier == 0:
                ended = step
                break
        step_block(f, previous_plan=True)
        done += 1
        fails += (ef < 0).sum()
        ee_clear = torch.minimum(ee_clear, store.box_distance(ee_of(tx), boxes))
        base_clear = torch.minimum(base_clear, store.box_distance(tx[:, :2], boxes))
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / max(done, 1)

    seen = (fmap.hits.long() + fmap.misses.long()) > 0
    truth = torch.from_numpy(raw > 0.5).to(dev)
    wrong = seen & ((fmap.occupancy(0.0, 1.0, 0.0) > 0.5) != truth)
    unseen_free = torch.nonzero(~seen & ~truth)
    replan_ms = event_ms(lambda: fg.replan(follower, tx), 20)
    out = dict(robots=B, steps=steps, K=K, rays=rays, fused=f["s"].is_fused(), nbox=int(len(boxes_np)),
               ended_step=ended, control_steps=done, replans=replans, frontier_cells=frontier,
               free_cells=int((~truth).sum().item()), free_cells_seen=int((seen & ~truth).sum().item()),
               unseen_free_cells=[(int(r), int(c)) for r, c in unseen_free.tolist()][:32],
               map_seen_cells=int(seen.sum().item()), map_wrong_cells=int(wrong.sum().item()),
               failed_solves=int(fails.item()), failed_share=int(fails.item()) / (B * max(done, 1)),
               min_ee_clearance_m=float(ee_clear.min().item()), min_base_clearance_m=float(base_clear.min().item()),
               base_inside=int((base_clear <= 0).sum().item()), ms_per_step=round(ms, 3),
               replan_ms=round(replan_ms, 4), r_body=store.R_BODY)
    f["s"].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--threshold", type=float, default=1.3)
    ap.add_argument("--replan-every", type=int, default=10)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.robots, a.steps, a.seed, K=a.K, rays=a.rays, threshold=a.threshold,
                         replan_every=a.replan_every)))


if __name__ == "__main__":
    main()
