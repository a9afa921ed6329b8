#!/usr/bin/env python3
"""Boxers exploring a store nobody has mapped, without goals: frontier exploration on the device.  The store, the
constants, the boxer model and ``LidarPlanes`` are those of examples/fleet_store_lidar.py (``BoxerStore`` of
robot_mpcs_amd/store.py); the robots start packed into one corner (``corner_starts``: the cells nearest it that are free on the map dilated by two cells) and nobody hands
them a goal.  Every control step, all on one stream:

    RouteFollower.step -> LidarPlanes.step -> FleetMap.mark -> solve_scene_device -> advance_device(..., exitflag=ef)

and at step 0 and every ``--replan-every`` steps, after the mark:

    FrontierGoals.replan -> frontier_cells()

``FrontierGoals.replan`` (robot_mpcs_amd/utils/exploration.py) classifies the evidence, enlarges the map, finds the
frontier -- the known free cells next to unknown space --, builds one cost-to-go field to the nearest frontier cell
and gives every robot the route down that field.  ``frontier_cells()`` is the loop's one host read: the run ends at the
first re-plan that finds no frontier, or after ``--steps`` control steps.  With ``--tile`` > 0 the robots are
coordinated instead: one target per tile of that many cells, a field per target, and a greedy assignment
of robots to targets by route cost, so that the fleet spreads over the frontier.

    python examples/fleet_store_frontier.py [--robots 64] [--steps 3000] [--seed 0] [--replan-every 10] [--tile 0]

Prints one JSON line: the step at which exploration ended (null if it did not), the store's free cells and those seen,
the seen cells and those among them classified against the true map, failed robot-steps, the least distance from the
end link and from the base centre to any shelf box, ms per control step, ms of ``FrontierGoals.replan`` (median of
20 event-timed calls) and ``tile`` (``run`` returns the same record without ``tile``).
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


def run(B=64, steps=3000, seed=0, dev="cuda:0", K=4, rays=64, threshold=1.3, replan_every=10, tile=0):
    import torch
    from robot_mpcs_amd.fleet import event_ms
    from robot_mpcs_amd.store import STORE, BoxerStore, map_errors, store_map
    from robot_mpcs_amd.utils.exploration import FrontierGoals, corner_starts

    rng = np.random.default_rng(seed)
    fleet = BoxerStore(B, seed, dev, K, rays, corner_starts(store_map(seed), B, STORE.clear_cells), rng)
    lp, tx = fleet.lp, fleet.x
    fmap = fleet.fleet_map()
    fg = FrontierGoals(fmap, STORE.size_robot, 0.29, tile=tile)
    follower = fleet.follower(threshold, max_len=fg.max_len)
    ended, replans, frontier = None, 0, None

    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    for step in range(steps):
        follower.step(tx, fleet.goal)
        fleet.scan()
        fmap.mark(tx, lp.points, lp.ranges)
        if step % replan_every == 0:
            fg.replan(follower, tx)
            replans += 1
            frontier = fg.frontier_cells()
            if frontier == 0:
                ended = step
                break
        fleet.drive()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / max(fleet.steps, 1)

    seen_cells, wrong_cells = map_errors(fmap, fleet.raw)
    seen = (fmap.hits.long() + fmap.misses.long()) > 0
    truth = torch.from_numpy(fleet.raw > 0.5).to(dev)
    unseen_free = torch.nonzero(~seen & ~truth)
    replan_ms = event_ms(lambda: fg.replan(follower, tx), 20)
    rep = fleet.report()
    out = dict({k: rep[k] for k in rep if k not in ("ee_clearance_p10", "ee_below_half_r_body")}, steps=steps,
               ended_step=ended, control_steps=fleet.steps, replans=replans, frontier_cells=frontier,
               free_cells=int((~truth).sum().item()), free_cells_seen=int((seen & ~truth).sum().item()),
               unseen_free_cells=[(int(r), int(c)) for r, c in unseen_free.tolist()][:32],
               map_seen_cells=seen_cells, map_wrong_cells=wrong_cells, ms_per_step=round(ms, 3),
               replan_ms=round(replan_ms, 4))
    fleet.close()
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
    ap.add_argument("--tile", type=int, default=0)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(dict(run(a.robots, a.steps, a.seed, K=a.K, rays=a.rays, threshold=a.threshold,
                              replan_every=a.replan_every, tile=a.tile), tile=a.tile)))


if __name__ == "__main__":
    main()
