#!/usr/bin/env python3
"""Boxers among walkers that they have to see for themselves, entirely on the device.  B boxers on the cfg3 model
(RadialConstraints with 5 moving obstacles, the fused kernel) drive to their goals in one open +-9 m arena in which P
walkers of radius 0.3 m bounce about (``rmpc_advance_obstacles_device(1, P, dt, 9.0, ...)``, at most 0.5 m/s per axis).
What the solver is told about the walkers is the mode:

    truth    each robot gets the five walkers nearest its sensor, by (distance^2, index), with their true velocity --
             what every loop with moving obstacles did so far (the simulator's state copied into obst_dyn);
    tracked  ``ObstacleTracker.step``: the robot's own 256-ray scan of the walkers within 6 m -> moving returns ->
             circle detections -> alpha-beta tracks in 16 slots -> the five nearest confirmed tracks;
    blind    every row parked: the robots do not know of the walkers.

Every control step, on one stream:  [tracker | nearest five]  ->  solve_scene_device  ->  advance_device  ->
rmpc_advance_obstacles_device.  Nothing crosses PCIe between control steps; the statistics stay on the device.  The
robots do not see each other here (the lidar world holds the walkers only); ``ObstacleTracker.step(..., bodies=...)``
puts the fleet into the scan, as examples/fleet_crossing_lidar.py --mode tracked does.

    python examples/fleet_moving_obstacles.py [--robots 64] [--walkers 24] [--steps 300] [--seed 0]
                                              [--obstacles truth|tracked|blind]

Prints one JSON line: the share of robot-steps in contact (end link to walker centre < r_body + 0.3), the least
clearance (that distance minus r_body + 0.3), the share of failed solves, arrivals, ms per control step (statistics
included); in tracked mode also the position and velocity error of the rows handed to the solver against the nearest
walker's truth (p50, p99, max), the share of walkers within 4 m of a sensor that have a confirmed track within 0.3 m, and
the share of the robot-steps in contact in which a row of obst_dyn lay within 0.3 m of the walker touched.
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

WALKER_RADIUS, WALKER_SPEED, ARENA, NOBST, PARK = 0.3, 0.5, 9.0, 5, (100.0, 100.0)
OFFSET = (0.4, 0.0)          # the boxer's end link and sensor, ahead of the base
# the filter of the tracked mode; run(..., alpha=0.6, beta=0.4, confirm=2, max_miss=10) is the quicker one of DESIGN.md 19
# (the solver extrapolates a row's velocity over its whole horizon, so a lagging velocity costs contacts)
TRACKER = dict(alpha=0.4, beta=0.1, confirm=3, max_miss=5, v_max=2.0 * WALKER_SPEED)


def place_walkers(rng, P, ee, r_body):
    """(P, 9) walkers in the arena, each at least WALKER_RADIUS + r_body + 1 from every end link ``ee`` (B, 2)"""
    w = np.zeros((P, 9))
    for q in range(P):
        while True:
            c = rng.uniform(-8.7, 8.7, 2)
            if np.linalg.norm(ee - c, axis=1).min() >= WALKER_RADIUS + r_body + 1.0:
                break
        w[q, :2] = c
    w[:, 3:5] = rng.uniform(-WALKER_SPEED, WALKER_SPEED, (P, 2))
    return w


def run(B=64, P=24, steps=300, seed=0, dev="cuda:0", obstacles="tracked", rays=256, n_tracks=16, track_range=6.0, **tracker_kw):
    import torch
    from robot_mpcs_amd import scenarios as sn
    from robot_mpcs_amd.fleet import Arrivals, MixedFleetShard, dev_f64, limit_tensors, make_block, step_block
    from robot_mpcs_amd.utils.tracking import ObstacleTracker

    if obstacles not in ("truth", "tracked", "blind"):
        raise ValueError("obstacles: truth, tracked or blind")
    sc = sn.make_scenario("cfg3", B=B, seed=seed)
    r_body, dt = float(sc.extra["r_body"]), float(sc.desc["dt"])
    rng = np.random.default_rng(seed + 77)
    ee0 = sc.xinit[:, :2] + OFFSET[0] * np.stack([np.cos(sc.xinit[:, 2]), np.sin(sc.xinit[:, 2])], axis=1)
    walkers = dev_f64(place_walkers(rng, P, ee0, r_body)[None], dev)          # (1, P, 9): one world for the fleet
    circles = torch.full((P, 3), WALKER_RADIUS, dtype=torch.float64, device=dev)

    tracker = None
    if obstacles == "tracked":
        tracker = ObstacleTracker(B, NOBST, rays=rays, n_tracks=n_tracks, radius=WALKER_RADIUS, dt=dt, offset=OFFSET,
                                  max_range=track_range, park=PARK, device=dev,
                                  **dict(TRACKER, **tracker_kw))
        obst_dyn = tracker.obst_dyn
    else:
        obst_dyn = torch.zeros((B, NOBST, 9), dtype=torch.float64, device=dev)
        obst_dyn[:, :, 0], obst_dyn[:, :, 1] = PARK
    f = make_block(sc.desc, sc.setup["mpc"]["weights"], B, sc.xinit, dev, x0=sc.x0, name="cfg3",
                   dyn_radius=WALKER_RADIUS, **limit_tensors(*sn.LIMITS["cfg3"], B, dev), goal=dev_f64(sc.extra["goal"], dev),
                   r_body=dev_f64(np.full(B, r_body), dev), obst_dyn=obst_dyn)
    goal2 = f["goal"][:, :2]
    tol = MixedFleetShard.ARRIVE_TOL["cfg3"]
    arrivals = Arrivals(B, dev)
    contact = torch.zeros((), dtype=torch.int64, device=dev)
    failed = torch.zeros((), dtype=torch.int64, device=dev)
    least = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    known = torch.zeros((), dtype=torch.int64, device=dev)
    perr, verr, seen, near = [], [], torch.zeros((), dtype=torch.int64, device=dev), torch.zeros((), dtype=torch.int64, device=dev)

    def sensor(x):
        return x[:, :2] + OFFSET[0] * torch.stack([torch.cos(x[:, 2]), torch.sin(x[:, 2])], dim=1)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(steps):
        w = walkers[0]
        o = sensor(f["x"])
        d = (o[:, None, :] - w[None, :, :2]).norm(dim=2)                      # (B, P): end link to walker centre
        contact += (d.min(dim=1).values < r_body + WALKER_RADIUS).sum()
        least = torch.minimum(least, d.min() - (r_body + WALKER_RADIUS))
        if obstacles == "truth":
            d2 = ((o[:, None, :] - w[None, :, :2]) ** 2).sum(dim=2)
            idx = torch.sort(d2, dim=1, stable=True).indices[:, :NOBST]       # (distance^2, index)
            n = idx.shape[1]
            obst_dyn[:, :n, 0:2] = w[idx][:, :, 0:2]
            obst_dyn[:, :n, 3:5] = w[idx][:, :, 3:5]
        elif obstacles == "tracked":
            circles[:, :2] = w[:, :2]
            tracker.step(f["x"], circles)
            rows = obst_dyn[:, :, 0] != PARK[0]                               # (B, 5): rows that hold a track
            dr = (obst_dyn[:, :, None, 0:2] - w[None, None, :, :2]).norm(dim=3)
            who = dr.argmin(dim=2)
            nan = torch.full_like(dr[:, :, 0], float("nan"))
            perr.append(torch.where(rows, dr.min(dim=2).values, nan))
            verr.append(torch.where(rows, (obst_dyn[:, :, 3:5] - w[who][:, :, 3:5]).norm(dim=2), nan))
            conf = tracker.age >= tracker.args.confirm                        # (B, T)
            dt_ = (tracker.track[:, None, :, :2] - w[None, :, None, :2]).norm(dim=3)        # (B, P, T)
            has = ((dt_ < 0.3) & conf[:, None, :]).any(dim=2)
            within = d < 4.0
            # a robot in contact: did a row of its obst_dyn hold the walker it touches?
            touch = d.min(dim=1).values < r_body + WALKER_RADIUS
            row_d = dr.gather(2, d.argmin(dim=1)[:, None, None].expand(-1, NOBST, 1))[:, :, 0]
            known += (touch & (torch.where(rows, row_d, torch.full_like(row_d, float("inf"))).min(dim=1).values < 0.3)).sum()
            near += within.sum()
            seen += (within & has).sum()
        step_block(f, previous_plan=True)
        failed += (f["ef"] < 0).sum()
        f["s"].advance_obstacles_device(walkers, dt, arena=ARENA)
        arrivals.update((sensor(f["x"]) - goal2).norm(dim=1) < tol, step)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps

    out = dict(robots=B, walkers=P, steps=steps, obstacles=obstacles, fused=bool(f["s"].is_fused()), r_body=r_body,
               contact_share=int(contact.item()) / (B * steps), least_clearance_m=float(least.item()),
               failed_share=int(failed.item()) / (B * steps), **arrivals.summary(), arrive_tol_m=tol,
               ms_per_step=round(ms, 3))
    if obstacles == "tracked":
        q = lambda a, p: float(np.nanpercentile(a, p)) if np.isfinite(a).any() else None
        pe, ve = torch.stack(perr).cpu().numpy(), torch.stack(verr).cpu().numpy()
        out.update(rays=rays, n_tracks=n_tracks, track_range_m=track_range, rows_tracked_share=float(np.isfinite(pe).mean()),
                   pos_err_p50=q(pe, 50), pos_err_p99=q(pe, 99), pos_err_max=q(pe, 100),
                   vel_err_p50=q(ve, 50), vel_err_p99=q(ve, 99), vel_err_max=q(ve, 100),
                   coverage_4m=int(seen.item()) / max(1, int(near.item())),
                   contact_known_share=int(known.item()) / max(1, int(contact.item())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=64)
    ap.add_argument("--walkers", type=int, default=24)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rays", type=int, default=256)
    ap.add_argument("--obstacles", choices=("truth", "tracked", "blind"), default="tracked")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.robots, a.walkers, a.steps, a.seed, obstacles=a.obstacles, rays=a.rays)))


if __name__ == "__main__":
    main()
