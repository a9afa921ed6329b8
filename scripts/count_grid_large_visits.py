#!/usr/bin/env python3
"""Tile visits of the large-map fields' work list counted in its numpy restatement
(tests/grid_large_reference.py), for both visit orders -- ascending / descending passes ("zigzag") and least key first
("least") -- on ``shelf_map(512, 512)`` and a 512 x 512 serpentine, with tiles of 32, 64 and 96 cells and 4 and 8 moves:
the counts the choice of the order and of the tile rests on.  Needs no GPU; takes some minutes.

    python scripts/count_grid_large_visits.py [--tiles 32,64,96] [--out profiles/grid_large_visit_counts.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", default="32,64,96")
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_large_visit_counts.json"))
    a = ap.parse_args()
    from global_planner_reference import field_ref
    from grid_large_reference import ORDERS, serpentine, tiled_field_ref
    from robot_mpcs_amd.global_planner.batch import shelf_map

    n = a.side
    store = shelf_map(n, n)
    free = np.flatnonzero(store.ravel() < 0.8)
    maps = (("shelf_map(%d, %d)" % (n, n), store, [int(free[0]), int(free[len(free) // 2]), int(free[-1])]),
            ("serpentine(%d, %d)" % (n, n), serpentine(n, n), [0, (n // 2) * n + 5]))
    rows = []
    for name, data, goals in maps:
        for movement in (4, 8):
            for goal in goals:
                ref = field_ref(data, goal, movement)
                for tile in (int(t) for t in a.tiles.split(",")):
                    r = dict(map=name, movement=movement, goal=goal, tile=tile, tiles=(-(-n // tile)) ** 2)
                    for order in ORDERS:
                        D, r[order] = tiled_field_ref(data, goal, tile, movement, order)
                        assert np.array_equal(D, ref)
                    rows.append(r)
                    print(json.dumps(r), flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(what="tile visits of tiled_field_ref, both orders", rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
