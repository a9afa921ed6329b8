#!/usr/bin/env python3
"""The crossing of examples/fleet_crossing.py (boxers on an open +-9 m floor whose straight lines cross), with no word
between the robots: what a robot knows of the others is what its own lidar returns.  Every robot is a round body of
radius r_body centred at its collision point (the end link, 0.4 m ahead of the base, where its sensor sits too), and
the scan sees the bodies of the others (``rmpc_lidar_scan_fleet_device``).  The mode is what the solver
is told:

    blind    dummy planes only: the shipped boxer model with K planes, its lidar in an empty world;
    seen     ``LidarPlanes(body_radius=r_body)``: fleet scan -> per-stage seeds -> free-space decomposition ->
             ``lin_constrs`` of the same model;
    tracked  the cfg3 model (five moving obstacles): ``ObstacleTracker(radius=r_body).step(..., bodies=...)``: fleet scan
             -> moving returns -> circle detections -> alpha-beta tracks -> ``obst_dyn``, with dyn_radius = r_body;
    truth    the cfg3 model told the five nearest robots' collision points and velocities: the privileged reference of
             ``tracked``, as in examples/fleet_moving_obstacles.py.

In seen, tracked and truth the solver keeps r_body + 0.2 m from what it is told (``MARGIN``): the others move between two
scans.  The distances reported are against r_i + r_j.

Every control step, on one stream:  [scan chain]  ->  solve_scene_device  ->  advance_device.  The goal each solve sees is
the look-ahead point of fleet_crossing.py.  Nothing crosses PCIe between control steps.

    python examples/fleet_crossing_lidar.py [--mode blind|seen|tracked|truth] [--robots 64] [--steps 400] [--seed 0] [--K 4]

Prints one JSON line with the fields of fleet_crossing.py: arrivals, the share of failed solves, the least distance
between two collision points against r_i + r_j (difference and ratio), the pair-steps closer than r_i + r_j - 1e-3 m, ms
per control step and ms of the scan chain alone (median of 20 event-timed calls).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from fleet_crossing import BELOW, ROBOTS, model, pick  # noqa: E402

MODES = ("blind", "seen", "tracked", "truth")
NOBST, PARK = 5, (100.0, 100.0)
# What the solver keeps from a plane or from a track's circle is r_body + MARGIN.  A scan is a snapshot: between two of
# them both robots of a pair move, each at up to about 1 m/s (the look-ahead goal's speed) for dt = 0.1 s, so a robot
# that plans up to r_body from where it saw the other stands up to 0.2 m inside r_i + r_j one step later -- and a hard
# constraint that starts violated has no feasible plan.  blind has nothing to keep a margin from.
MARGIN = dict(blind=0.0, seen=0.2, tracked=0.2, truth=0.2)
# The tracked mode's scan and filter.  1024 rays out to 4 m: a circle of 8 m across holds about ten of 64 robots on the
# +-9 m floor, which fits the 16 slots (a slot held by a far robot is one a near robot cannot be born into, DESIGN.md
# 19).  Two returns link below gap = 0.3 m: neighbouring returns on one body of radius 0.6 at 4 m are at most
# sqrt(2 r (4 * 2 pi / 1024)) = 0.17 m apart (the step onto the rim), and bodies whose surfaces are farther apart than
# the gap stay two segments (the tracker's default, 1.5 radius = 0.9 m, joins robots that stand side by side into one
# segment wider than max_extent, which is dropped).  The filter is the quicker one of DESIGN.md 19 (the solver
# extrapolates a row's velocity over its horizon); velocities are held within twice the look-ahead goal's speed.
TRACK = dict(rays=1024, n_tracks=16, max_range=4.0, gap=0.3, alpha=0.6, beta=0.4, confirm=2, max_miss=10, v_max=2.0)


def run(mode="seen", B=None, steps=None, seed=0, K=4, dev="cuda:0", lookahead=None, margin=None, **track_kw):
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd import scenarios as sn
    from robot_mpcs_amd.fleet import Arrivals, dev_f64, event_ms, limit_tensors, make_block, step_block
    from robot_mpcs_amd.utils.lidar import LidarPlanes
    from robot_mpcs_amd.utils.tracking import ObstacleTracker

    if mode not in MODES:
        raise ValueError("mode: blind, seen, tracked or truth")
    cfg = ROBOTS["boxer"]
    B, steps, r = int(B or cfg["B"]), int(steps or cfg["steps"]), cfg["r_body"]
    rng = np.random.default_rng(seed)
    base, th, goals = pick(B, r, rng, cfg["heading"], cfg["offset"])
    rad = dev_f64(np.full(B, r), dev)
    margin = float(MARGIN[mode] if margin is None else margin)
    keep = dev_f64(np.full(B, r + margin), dev)          # what the solver keeps from a plane or from a track's circle
    goal = dev_f64(np.concatenate([goals, np.zeros((B, 1))], 1), dev)
    if mode in ("tracked", "truth"):
        sc = sn.make_scenario("cfg3", B=1, seed=seed)
        desc, setup, (lim, limu) = sc.desc, sc.setup, sn.LIMITS["cfg3"]
    else:
        desc, setup, lim, limu = model("boxer", B, K, seed)
    N = desc["N"]
    xinit = np.zeros((B, desc["nx"]))
    xinit[:, :2], xinit[:, 2] = base, th
    if mode == "truth":
        dt = float(desc["dt"])
        obst_dyn = torch.zeros((B, NOBST, 9), dtype=torch.float64, device=dev)
        obst_dyn[:, :, 0], obst_dyn[:, :, 1] = PARK
        f = make_block(desc, setup["mpc"]["weights"], B, xinit, dev, name="cfg3", goal=goal, r_body=keep, dyn_radius=r,
                       obst_dyn=obst_dyn, **limit_tensors(lim, limu, B, dev))
        last = []

        def chain(x, z, ef):
            c = x[:, :2] + cfg["offset"][0] * torch.stack([torch.cos(x[:, 2]), torch.sin(x[:, 2])], 1)
            v = (c - last[0]) / dt if last else torch.zeros_like(c)
            last[:] = [c]
            d2 = ((c[:, None, :] - c[None, :, :]) ** 2).sum(dim=2)
            d2.fill_diagonal_(float("inf"))
            idx = torch.sort(d2, dim=1, stable=True).indices[:, :NOBST]
            obst_dyn[:, :, 0:2], obst_dyn[:, :, 3:5] = c[idx], v[idx]
    elif mode == "tracked":
        centres = torch.zeros((B, 1, 3), dtype=torch.float64, device=dev)
        tracker = ObstacleTracker(B, NOBST, radius=r, dt=float(desc["dt"]), offset=cfg["offset"], park=PARK, device=dev,
                                  **dict(TRACK, **track_kw))
        f = make_block(desc, setup["mpc"]["weights"], B, xinit, dev, name="cfg3", goal=goal, r_body=keep, dyn_radius=r,
                       obst_dyn=tracker.obst_dyn, **limit_tensors(lim, limu, B, dev))

        def chain(x, z, ef):
            _lib.fleet_points_device(x, centres, None, None, cfg["heading"], cfg["offset"], 0.0)
            tracker.step(x, None, bodies=(centres, rad, 0))
    else:
        lp = LidarPlanes(B, N, K, offset=cfg["offset"], device=dev, body_radius=r if mode == "seen" else None,
                         heading=cfg["heading"])
        f = make_block(desc, setup["mpc"]["weights"], B, xinit, dev, goal=goal, r_body=keep, lin_constrs=lp.planes,
                       **limit_tensors(lim, limu, B, dev))

        def chain(x, z, ef):
            lp.step(x, z, ef)
    previous_plan = setup["mpc"].get("initialization", "previous_plan") == "previous_plan"
    lookahead = float(cfg["lookahead"] if lookahead is None else lookahead)
    final = goal.clone()
    tx, z, ef = f["x"], f["z"], f["ef"]

    def cpoint(x):
        return x[:, :2] + cfg["offset"][0] * torch.stack([torch.cos(x[:, 2]), torch.sin(x[:, 2])], 1)

    upper = torch.triu(torch.ones((B, B), dtype=torch.bool, device=dev), diagonal=1)
    rsum = rad[:, None] + rad[None, :]
    inf = torch.full((B, B), float("inf"), dtype=torch.float64, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    fails, flag0, below = torch.zeros((), **i64), torch.zeros((), **i64), torch.zeros((), **i64)
    min_gap = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    min_ratio = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    arrivals = Arrivals(B, dev)
    near, tracked_near = torch.zeros((), **i64), torch.zeros((), **i64)
    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    for step in range(steps):
        p0 = cpoint(tx)
        dg = final[:, :2] - p0
        goal[:, :2] = p0 + dg * torch.clamp(lookahead / torch.clamp(dg.norm(dim=1, keepdim=True), min=1e-12), max=1.0)
        chain(tx, z if step > 0 else None, ef if step > 0 else None)
        if mode == "tracked":
            # the robots within 3 m of a sensor that have a confirmed track within 0.3 m of their collision point
            conf = tracker.age >= tracker.args.confirm
            dt_ = (tracker.track[:, None, :, :2] - p0[None, :, None, :]).norm(dim=3)          # (B, B, T)
            within = ((p0[:, None, :] - p0[None, :, :]).norm(dim=2) < 3.0) & ~torch.eye(B, dtype=torch.bool, device=dev)
            near += within.sum()
            tracked_near += (within & ((dt_ < 0.3) & conf[:, None, :]).any(dim=2)).sum()
        step_block(f, previous_plan)
        fails += (ef < 0).sum()
        flag0 += (ef == 0).sum()
        p = cpoint(tx)
        d = (p[:, None, :] - p[None, :, :]).norm(dim=2)
        min_gap = torch.minimum(min_gap, torch.where(upper, d - rsum, inf).min())
        min_ratio = torch.minimum(min_ratio, torch.where(upper, d / rsum, inf).min())
        below += (torch.where(upper, d - rsum, inf) < -BELOW).sum()
        arrivals.update((p - final[:, :2]).norm(dim=1) < cfg["tol"], step)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / steps

    scan_ms = event_ms(lambda: chain(tx, z, ef), 20)
    out = dict(mode=mode, robots=B, steps=steps, K=K if mode in ("blind", "seen") else None, seed=seed, N=N, r_body=r,
               lookahead=lookahead, fused=bool(f["s"].is_fused()), **arrivals.summary(),
               failed_solves=int(fails.item()), failed_share=int(fails.item()) / (B * steps), flag0_solves=int(flag0.item()),
               min_gap_m=float(min_gap.item()), min_ratio=float(min_ratio.item()), below_pair_steps=int(below.item()),
               ms_per_step=round(ms, 3), scan_chain_ms=round(scan_ms, 4),
               arrive_tol_m=cfg["tol"], margin_m=margin)
    if mode == "tracked":
        out.update(coverage_3m=int(tracked_near.item()) / max(1, int(near.item())),
                   **{k: v for k, v in dict(TRACK, **track_kw).items()})
    f["s"].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=MODES, default="seen")
    ap.add_argument("--robots", type=int, default=None)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--K", type=int, default=4)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.mode, a.robots, a.steps, a.seed, a.K)))


if __name__ == "__main__":
    main()
