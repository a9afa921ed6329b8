#!/usr/bin/env python3
"""Throughput of the global planner on one GPU, on seeded shelf maps of 41 x 41 (the reference's occupancy sensor,
examples/boxer_example_global.py) and 128 x 128 cells (the largest field kept in LDS), enlarged as the example does:

  - fields/s for G = 1, 16, 64 goals per launch (rmpc_grid_fields_device), with the sweeps the fields took;
  - the time of 4096 path queries over 16 fields (rmpc_grid_paths_device);
  - the follower's time per control step at B = 4096 (rmpc_follow_path_device);
  - a single-thread CPU heap A* (the reference's algorithm, in Python, on this machine's host CPU) per query.
    It ran on the same box as the GPU, so it is a yardstick of the scale, not a tuned CPU baseline.

    timeout -k 10 300 python scripts/bench_global_planner.py [--reps 20]

Prints one JSON line.  Times are medians over --reps launches, each synchronised (CUDA events).
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


def cpu_astar_ms(grid, pairs):
    """Median ms per query of a heap A* with the reference's priority (g + h + potential twice)."""
    import heapq
    import math
    H, W = grid.shape
    s2 = math.sqrt(2)
    moves = [(1, 0, 1.0), (0, 1, 1.0), (-1, 0, 1.0), (0, -1, 1.0), (1, 1, s2), (-1, 1, s2), (-1, -1, s2), (1, -1, s2)]
    times = []
    for s, g in pairs:
        start, goal = (s % W, s // W), (g % W, g // W)
        t0 = time.perf_counter()
        visited = np.zeros((H, W), bool)
        front = [(math.dist(start, goal), 0.0, start)]
        while front:
            _, cost, pos = heapq.heappop(front)
            if visited[pos[1], pos[0]]:
                continue
            visited[pos[1], pos[0]] = True
            if pos == goal:
                break
            for dx, dy, dc in moves:
                n = (pos[0] + dx, pos[1] + dy)
                if 0 <= n[0] < W and 0 <= n[1] < H and not visited[n[1], n[0]] and grid[n[1], n[0]] < 0.8:
                    pot = grid[n[1], n[0]] * 3.0
                    nc = cost + dc + pot
                    heapq.heappush(front, (nc + math.dist(n, goal) + pot, nc, n))
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import event_ms
    from robot_mpcs_amd.global_planner import RouteFollower, shelf_map

    dev = "cuda:0"
    rng = np.random.default_rng(0)
    res = {}
    for H, cell in ((41, 0.45), (128, 0.15)):
        raw = torch.from_numpy(shelf_map(H, H, seed=1, aisle=4 if H == 41 else 9, shelf=2 if H == 41 else 4,
                                         gap=3 if H == 41 else 6)).to(dev)
        grid = torch.empty_like(raw)
        _lib.grid_inflate_device(raw, grid, cell, 0.45, 0.29)
        free = np.flatnonzero(grid.cpu().numpy().ravel() < 0.8)
        r = {}
        for G in (1, 16, 64):
            goals = torch.from_numpy(rng.choice(free, G, replace=False).astype(np.int32)).to(dev)
            fields = torch.empty((G, H, H), dtype=torch.float64, device=dev)
            status = torch.empty(G, dtype=torch.int32, device=dev)
            sweeps = torch.empty(G, dtype=torch.int32, device=dev)
            ms = event_ms(lambda: _lib.grid_fields_device(grid, goals, fields, status, sweeps=sweeps), a.reps)
            r[f"fields_G{G}_ms"] = round(ms, 4)
            r[f"fields_G{G}_per_s"] = round(1e3 * G / ms, 1)
            r[f"sweeps_G{G}_max"] = int(sweeps.max().item())
        Bq = 4096
        gi = torch.from_numpy(rng.integers(0, 16, Bq).astype(np.int32)).to(dev)
        starts = torch.from_numpy(rng.choice(free, Bq).astype(np.int32)).to(dev)
        goals16 = goals[:16].contiguous()
        fields16 = fields[:16].contiguous()
        max_len = 4 * (2 * H)
        path = torch.empty((Bq, max_len), dtype=torch.int32, device=dev)
        lens = torch.empty(Bq, dtype=torch.int32, device=dev)
        r["paths_4096_ms"] = round(event_ms(lambda: _lib.grid_paths_device(grid, fields16, goals16, starts, gi, path, lens),
                                         a.reps), 4)
        r["path_len_max"] = int(lens.max().item())
        f = RouteFollower(path, lens, H, -1.0, -1.0, cell)
        xinit = torch.zeros((Bq, 6), dtype=torch.float64, device=dev)
        goal = torch.zeros((Bq, 3), dtype=torch.float64, device=dev)
        r["follow_4096_us"] = round(1e3 * event_ms(lambda: f.step(xinit, goal), a.reps * 5), 2)
        pairs = [(int(s), int(goals16[int(k)].item())) for s, k in zip(starts[:32].cpu().numpy(), gi[:32].cpu().numpy())]
        r["cpu_astar_ms_per_query"] = round(cpu_astar_ms(grid.cpu().numpy(), pairs), 3)
        res[f"{H}x{H}"] = r
    print(json.dumps(dict(bench="global_planner", device=torch.cuda.get_device_name(0), results=res)))


if __name__ == "__main__":
    main()
