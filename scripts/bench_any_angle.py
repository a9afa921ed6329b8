#!/usr/bin/env python3
"""Line of sight, shortened routes and the follower that looks ahead (include/rmpc_any_angle.h) on one
GPU, on the seeded shelf maps of scripts/bench_global_planner.py (41 x 41 and 128 x 128 cells, enlarged with
size_robot = 0.45), B = 4096 routes over 16 fields:

  - rmpc_grid_shorten_device with reach 0 and 16, and rmpc_grid_paths_device on the same routes beside it (for scale);
  - rmpc_follow_visible_device with reach 16 and 64, and the parent's rmpc_follow_path_device on the same inputs: every
    robot stands on the cell a third of the way along its route, with that index, reset before every launch;
  - 1e6 pairs of rmpc_grid_visible_device;
  - the control step of examples/fleet_global_route.py (256 robots, 200 steps) with either follower, in the same run,
    against which the follower's time is held (--no-loop skips it).

    timeout -k 10 600 python scripts/bench_any_angle.py [--reps 20] [--out profiles/any_angle_bench.json]

Every time is the median of --reps event-timed launches after a warm one, with the least and the greatest beside it.
Writes the JSON to --out and prints it.  No time is gated.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(torch, fn, reps, before=None):
    """ms: (median, least, greatest) of reps launches of fn, each between two events, `before` outside them"""
    out = []
    for k in range(reps + 1):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        if k:
            out.append(a.elapsed_time(b))
    return dict(ms=round(float(np.median(out)), 5), least=round(min(out), 5), greatest=round(max(out), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-loop", action="store_true", help="skip the example's control step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "any_angle_bench.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from example_loader import load_example
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.global_planner import route_lengths, shelf_map

    dev = "cuda:0"
    rng = np.random.default_rng(0)
    B, res = 4096, {}
    for H, cell in ((41, 0.45), (128, 0.15)):
        raw = torch.from_numpy(shelf_map(H, H, seed=1, aisle=4 if H == 41 else 9, shelf=2 if H == 41 else 4,
                                         gap=3 if H == 41 else 6)).to(dev)
        grid = torch.empty_like(raw)
        _lib.grid_inflate_device(raw, grid, cell, 0.45, 0.29)
        free = np.flatnonzero(grid.cpu().numpy().ravel() < 0.8)
        goals = torch.from_numpy(rng.choice(free, 16, replace=False).astype(np.int32)).to(dev)
        fields = torch.empty((16, H, H), dtype=torch.float64, device=dev)
        status = torch.empty(16, dtype=torch.int32, device=dev)
        _lib.grid_fields_device(grid, goals, fields, status)
        gi = torch.from_numpy(rng.integers(0, 16, B).astype(np.int32)).to(dev)
        starts = torch.from_numpy(rng.choice(free, B).astype(np.int32)).to(dev)
        max_len = 8 * H
        path = torch.zeros((B, max_len), dtype=torch.int32, device=dev)
        lens = torch.empty(B, dtype=torch.int32, device=dev)
        r = dict(paths=timed(torch, lambda: _lib.grid_paths_device(grid, fields, goals, starts, gi, path, lens), a.reps))
        r["routes"], r["route_cells"], r["route_cells_max"] = int((lens > 0).sum()), int(lens.clamp(min=0).sum()), int(lens.max())
        r["route_m"] = round(float(route_lengths(path, lens, H, cell).sum()), 2)

        out, out_len, src = torch.zeros_like(path), torch.empty_like(lens), torch.zeros_like(path)
        work = torch.empty(_lib.shorten_work_bytes(H, H) // 4, dtype=torch.int32, device=dev)
        for reach in (0, 16):
            fn = lambda: _lib.grid_shorten_device(grid, path, lens, out, out_len, work, reach=reach, src=src)
            r["shorten_reach%d" % reach] = dict(timed(torch, fn, a.reps), cells=int(out_len.clamp(min=0).sum()),
                                                metres=round(float(route_lengths(out, out_len, H, cell).sum()), 2))

        at = (lens.clamp(min=1) - 1) // 3
        c = path.gather(1, at[:, None].long())[:, 0]
        xinit = torch.zeros((B, 6), dtype=torch.float64, device=dev)
        xinit[:, 0], xinit[:, 1] = -1.0 + (c % H).double() * cell, -1.0 + (c // H).double() * cell
        idx, goal = at.clone().contiguous(), torch.zeros((B, 3), dtype=torch.float64, device=dev)
        blocked = torch.zeros(B, dtype=torch.int32, device=dev)
        reset = lambda: idx.copy_(at)
        look = 1.75 * cell / 0.45                                           # the example's look-ahead in cells
        r["follow_path"] = timed(torch, lambda: _lib.follow_path_device(path, lens, idx, xinit, goal, H, -1.0, -1.0, cell,
                                                                        1.3 * cell / 0.45), a.reps, reset)
        for reach in (16, 64):
            fn = lambda: _lib.follow_visible_device(path, lens, idx, xinit, goal, grid, -1.0, -1.0, cell, reach=reach,
                                                    look_ahead=look, blocked=blocked)
            r["follow_visible_reach%d" % reach] = dict(timed(torch, fn, a.reps, reset), advance_mean=round(float((idx - at).double().mean()), 2),
                                                       blocked=int(blocked.sum()))
            # without the distance test every candidate is walked
            fn = lambda: _lib.follow_visible_device(path, lens, idx, xinit, goal, grid, -1.0, -1.0, cell, reach=reach,
                                                    look_ahead=1e6, blocked=blocked)
            r["follow_visible_reach%d_no_distance" % reach] = dict(timed(torch, fn, a.reps, reset),
                                                                   advance_mean=round(float((idx - at).double().mean()), 2))

        P = 1000000
        pa, pb = (torch.from_numpy(rng.choice(free, P).astype(np.int32)).to(dev) for _ in range(2))
        vis = torch.empty(P, dtype=torch.int32, device=dev)
        r["visible_1e6_pairs"] = dict(timed(torch, lambda: _lib.grid_visible_device(grid, pa, pb, vis), a.reps),
                                      visible_share=round(float((vis == 1).double().mean()), 4))
        res["%dx%d" % (H, H)] = r
        print(json.dumps({"%dx%d" % (H, H): r}), flush=True)

    loop = {}
    if not a.no_loop:
        ex = load_example("fleet_global_route")
        for name in ("waypoint", "visible"):
            rep = ex.run(B=256, steps=200, seed=0, follower=name)
            loop[name] = dict(ms_per_step=rep["ms_per_step"], failed_solves=rep["failed_solves"])
        tenth = 0.1 * loop["waypoint"]["ms_per_step"]
        loop["tenth_of_the_waypoint_step_ms"] = round(tenth, 4)
        loop["follow_visible_reach16_below_it"] = bool(res["41x41"]["follow_visible_reach16"]["ms"] < tenth)
    out = dict(bench="any_angle", device=torch.cuda.get_device_name(0), reps=a.reps, B=B, source_hash=_lib.source_hash(),
               results=res, control_step=loop)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
