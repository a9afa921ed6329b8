#!/usr/bin/env python3
"""Cost-to-go fields on maps beyond one workgroup's LDS (rmpc_grid_fields_large_device) on one GPU:
seeded ``shelf_map`` stores of 256^2, 512^2, 1024^2 and 2048^2 cells, G = 1, 16, 64, 256 goals per launch, 4 and 8
moves; per case the median of --reps event-timed calls (after one warm call), the tile visits per field, and beside
them the LDS entry (rmpc_grid_fields_device) on 128^2 at the same G and the host time of the heap Dijkstra
``field_ref`` (tests/global_planner_reference.py, single-thread Python on the machine the GPU sits in: a yardstick of
the scale, not a tuned CPU baseline) for one goal, against which the first field of the G = 1 launch with 8 moves is
compared bit for bit.

    timeout -k 10 900 python scripts/bench_grid_large.py [--reps 5] [--sides 256,512,1024,2048] [--out profiles/grid_large_bench.json]

Writes the JSON to --out and prints one progress line per case and the JSON at the end.  No time is gated.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GS = (1, 16, 64, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sides", default="256,512,1024,2048")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_large_bench.json"))
    ap.add_argument("--no-host", action="store_true", help="skip field_ref (its time and the bitwise comparison)")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from global_planner_reference import field_ref
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import event_ms
    from robot_mpcs_amd.global_planner import shelf_map

    dev = "cuda:0"
    rows = []

    def case(entry, side, movement, G, grid, free, rng, host):
        goals_np = rng.choice(free, G, replace=False).astype(np.int32)
        goals = torch.from_numpy(goals_np).to(dev)
        fields = torch.empty((G, side, side), dtype=torch.float64, device=dev)
        status = torch.empty(G, dtype=torch.int32, device=dev)
        count = torch.empty(G, dtype=torch.int32, device=dev)
        large = entry == "large"
        fn = (lambda: _lib.grid_fields_large_device(grid, goals, fields, status, movement, visits=count)) if large else \
            (lambda: _lib.grid_fields_device(grid, goals, fields, status, movement, sweeps=count))
        ms = event_ms(fn, a.reps)
        assert int((status != 0).sum().item()) == 0, status
        n = count.cpu().numpy()
        r = dict(entry=entry, side=side, cells=side * side, movement=movement, G=G, ms=round(ms, 4),
                 fields_per_s=round(1e3 * G / ms, 2), **{("visits" if large else "sweeps") + "_mean": round(float(n.mean()), 1),
                                                         ("visits" if large else "sweeps") + "_max": int(n.max())})
        if large:
            r["tiles"] = _lib.grid_tiles(side, side, _lib.GRID_TILE)
        if host and G == 1 and movement == 8:
            t0 = time.perf_counter()
            ref = field_ref(grid.cpu().numpy(), int(goals_np[0]), movement)
            r["field_ref_host_s"] = round(time.perf_counter() - t0, 3)
            r["equals_field_ref"] = bool(np.array_equal(fields[0].cpu().numpy(), ref))
        rows.append(r)
        print(json.dumps(r), flush=True)

    for entry, sides in (("lds", [128]), ("large", [int(s) for s in a.sides.split(",")])):
        for side in sides:
            grid = torch.from_numpy(shelf_map(side, side, seed=1, aisle=9, shelf=4, gap=6)).to(dev)
            free = np.flatnonzero(grid.cpu().numpy().ravel() < 0.8)
            for movement in (8, 4):
                rng = np.random.default_rng(side)
                for G in GS:
                    case(entry, side, movement, G, grid, free, rng, not a.no_host)
    out = dict(bench="grid_large", device=torch.cuda.get_device_name(0), reps=a.reps, tile=_lib.GRID_TILE,
               workgroup_threads=1024, order="ascending / descending passes", source_hash=_lib.source_hash(), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
