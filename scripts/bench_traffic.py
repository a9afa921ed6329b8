#!/usr/bin/env python3
"""Traffic-aware routes (include/rmpc_traffic.h) on one GPU, on seeded shelf maps of 41 x 41 (the store)
and 128 x 128 cells (the limit):

  - rmpc_grid_fields_traffic_device at G = 1, 16, 64 goals on the flow table of 256 blind routes, with the sweeps the
    slowest field took, and beside it in the same run the yardstick: rmpc_grid_fields_device (fp64, cost factor 3) for
    the same goals on the same map;
  - rmpc_grid_paths_traffic_device, rmpc_grid_traffic_add_device and rmpc_grid_traffic_score_device at B = 64, 256, 4096
    robots bound for 64 distinct goals;
  - ``TrafficRoutes.plan`` at the same B with 2 rounds, in 1 group and in 8, with the score (L, V, C) of every round.

    timeout -k 10 600 python scripts/bench_traffic.py [--reps 20] [--out profiles/traffic_bench.json]

Every time is the median of --reps event-timed launches after a warm one, with the least and the greatest beside it.
Writes the JSON to --out and prints it.  No time is gated.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(torch, fn, reps):
    """ms: (median, least, greatest) of reps launches of fn, each between two events, after a warm one"""
    out = []
    for k in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        if k:
            out.append(a.elapsed_time(b))
    return dict(ms=round(float(np.median(out)), 5), least=round(min(out), 5), greatest=round(max(out), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traffic_bench.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.global_planner import TrafficRoutes, shelf_map

    dev = "cuda:0"
    i32 = dict(dtype=torch.int32, device=dev)
    costs = _lib.traffic_costs()
    res = {}
    for H in (41, 128):
        k = max(1, H // 41)
        raw = shelf_map(H, H, seed=1, aisle=4 * k, shelf=2 * k, gap=3 * k)
        grid = torch.from_numpy(raw).to(dev)
        rng = np.random.default_rng(H)
        free = np.flatnonzero(raw.ravel() < 0.5)
        picks = rng.choice(free, 64, replace=False).astype(np.int32)
        fleets = {B: (rng.choice(free, B).astype(np.int32), picks[rng.integers(0, 64, B)]) for B in (64, 256, 4096)}
        out = res["%dx%d" % (H, H)] = dict(free_cells=int(len(free)), fields={}, entries={}, plan={})

        # the table the fields are timed on: 256 blind routes
        blind = TrafficRoutes(grid, *fleets[256], costs=costs, rounds=0, device=dev)
        blind.plan()
        flow = blind.flow.clone()
        for G in (1, 16, 64):
            goals = torch.from_numpy(picks[:G]).to(dev)
            fields, status, sweeps = torch.empty((G, H, H), **i32), torch.empty(G, **i32), torch.empty(G, **i32)
            fields64 = torch.empty((G, H, H), dtype=torch.float64, device=dev)
            t = timed(torch, lambda: _lib.grid_fields_traffic_device(grid, flow, costs, goals, fields, status, 8, 0.8, sweeps=sweeps), a.reps)
            mine = dict(t, sweeps_max=int(sweeps.max()), status_ok=bool((status == 0).all()))
            t = timed(torch, lambda: _lib.grid_fields_device(grid, goals, fields64, status, 8, 0.8, 3.0, sweeps=sweeps), a.reps)
            out["fields"]["G%d" % G] = dict(traffic=mine, grid_fields_fp64=dict(t, sweeps_max=int(sweeps.max())))
        print(json.dumps({"%dx%d" % (H, H): dict(fields=out["fields"])}), flush=True)

        sorted_goals = torch.from_numpy(np.sort(picks)).to(dev)
        fields, status = torch.empty((64, H, H), **i32), torch.empty(64, **i32)
        _lib.grid_fields_traffic_device(grid, flow, costs, sorted_goals, fields, status, 8, 0.8)
        score = torch.zeros(3, dtype=torch.int64, device=dev)
        max_len = min(H * H, 8 * H)
        for B, (starts, ends) in fleets.items():
            s, index = torch.from_numpy(starts).to(dev), torch.from_numpy(np.searchsorted(np.sort(picks), ends).astype(np.int32)).to(dev)
            path, length = torch.zeros((B, max_len), **i32), torch.zeros(B, **i32)
            table = torch.zeros_like(flow)
            e = dict(paths=timed(torch, lambda: _lib.grid_paths_traffic_device(grid, flow, costs, fields, sorted_goals, s, index, path,
                                                                                length, 8, 0.8), a.reps))
            e["mean_route_cells"] = round(float(length.double().mean()), 1)
            e["add"] = timed(torch, lambda: _lib.grid_traffic_add_device(table, path, length, 1), a.reps)
            e["score"] = timed(torch, lambda: _lib.grid_traffic_score_device(table, score, costs.base_axial, costs.base_diag), a.reps)
            out["entries"]["B%d" % B] = e
            for J in (1, 8):
                tr = TrafficRoutes(grid, starts, ends, costs=costs, groups=J, rounds=2, device=dev)
                t = timed(torch, tr.plan, max(3, a.reps // 4))
                out["plan"]["B%d_groups%d" % (B, J)] = dict(t, rounds=2, scores_LVC=tr.scores.cpu().tolist(),
                                                           routes=int((tr.lens > 0).sum()))
        print(json.dumps({"%dx%d" % (H, H): dict(entries=out["entries"], plan=out["plan"])}), flush=True)
    full = dict(bench="traffic", device=torch.cuda.get_device_name(0), reps=a.reps, source_hash=_lib.source_hash(),
                costs={f: getattr(costs, f) for f, _ in costs._fields_ if f != "struct_size"}, **res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(full, f, indent=1)
        f.write("\n")
    print(json.dumps(full))


if __name__ == "__main__":
    main()
