#!/usr/bin/env python3
"""Time of the timed tours' plan on one GPU at the shapes of section 18's table: the examples' store
(41 x 41 cells, T = 128: the history in LDS) and a 128 x 128 store (T = 256: in the workspace), B = 16, 64, 256 robots,
G = 1, 16, 64 priority orders; per shape ``rmpc_timed_plan_device`` (one goal per robot: its first stop) and
``rmpc_timed_tours_plan_device`` with K = 1, 2, 8 stops per robot and dwell 0 and 4, all on the same fields, in one
session.  Starts are distinct random cells that the enlarged map calls free; the stops of a robot are K of 4 B such
cells drawn at random, and it parks by the last; sep2 = 9, lag = 1, movement 4.  Random stops across the map do not fit
every window: the best order's unserved stops and failed robots are reported beside the time.

Times are medians of --reps event-timed calls (each synchronised), after one warm-up call.

    timeout -k 10 900 python scripts/bench_timed_tours.py [--reps 5] [--out profiles/timed_tours_bench.json]

Writes one JSON document to --out and prints it.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STOPS, DWELLS = (1, 2, 8), (0, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timed_tours_bench.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import event_ms
    from robot_mpcs_amd.global_planner import png_values, priority_orders, shelf_map
    from robot_mpcs_amd.store import STORE as S

    dev, i32 = "cuda:0", torch.int32
    rng = np.random.default_rng(0)
    out = {}
    new = lambda *s, dt=i32: torch.empty(s, dtype=dt, device=dev)
    for H, T, kw in ((S.H, 128, dict(aisle=S.aisle, shelf=S.shelf, gap=S.gap)), (128, 256, dict(aisle=9, shelf=4, gap=6))):
        raw = shelf_map(H, H, seed=0, **kw)
        g_raw = torch.from_numpy(png_values(raw)).to(dev)
        g_inf = torch.empty_like(g_raw)
        _lib.grid_inflate_device(g_raw, g_inf, S.cell, S.size_robot, 0.29)
        free = np.flatnonzero(g_inf.cpu().numpy().ravel() < 0.8)
        for B in (16, 64, 256):
            Gf = min(4 * B, len(free) - B)
            cells = rng.choice(free, B + Gf, replace=False).astype(np.int32)
            starts, picks = torch.from_numpy(cells[:B]).to(dev), torch.from_numpy(cells[B:]).to(dev)
            fields, fstat = new(Gf, H, H, dt=torch.float64), new(Gf)
            _lib.grid_fields_device(g_inf, picks, fields, fstat, 4, 0.8, 3.0)
            all_stops = np.stack([rng.choice(Gf, max(STOPS), replace=False) for _ in range(B)]).astype(np.int32)
            for G in (1, 16, 64):
                orders = torch.from_numpy(priority_orders(B, G, 0)).to(dev)
                work = new(_lib.timed_tours_work_bytes(H, H, T, G), dt=torch.uint8)
                paths, status, arrive, served = new(G, B, T + 1), new(G, B), new(G, B), new(G, B)
                key, best, unserved = new(G, dt=torch.int64), new(1), new(G)
                first = torch.from_numpy(all_stops[:, 0].copy()).to(dev)
                pa = _lib.timed_plan_args(g_inf, starts, first, fields, picks, orders, work, paths, status, arrive, key, best,
                                          movement=4, occ_threshold=0.8, sep2=9, lag=1)
                _lib.timed_plan_device(pa)
                r = dict(timed_plan_ms=round(event_ms(lambda: _lib.timed_plan_device(pa), a.reps), 3))
                r["timed_plan_best_failures"] = int((status[int(best.item())] > 0).sum().item())
                for K in STOPS:
                    stops = torch.from_numpy(all_stops[:, :K].copy()).to(dev)
                    lens = torch.full((B,), K, dtype=i32, device=dev)
                    park = stops[:, K - 1].contiguous()
                    serve_at = new(G, B, K)
                    for dwell in DWELLS:
                        ta = _lib.timed_tours_args(g_inf, starts, stops, lens, park, fields, picks, orders, work, paths, status,
                                                   arrive, key, best, serve_at, served, unserved, dwell=dwell, movement=4,
                                                   occ_threshold=0.8, sep2=9, lag=1)
                        _lib.timed_tours_plan_device(ta)
                        ms = event_ms(lambda: _lib.timed_tours_plan_device(ta), a.reps)
                        b = int(best.item())
                        r[f"K{K}_dwell{dwell}"] = dict(plan_ms=round(ms, 3), best_order=b, stops=B * K,
                                                       best_unserved=int(unserved[b].item()),
                                                       best_failures=int((status[b] > 0).sum().item()))
                out[f"{H}x{H}_T{T}_B{B}_G{G}"] = r
    doc = dict(bench="timed_tours", device=torch.cuda.get_device_name(0), reps=a.reps, sep2=9, lag=1, movement=4, cases=out)
    text = json.dumps(doc, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
