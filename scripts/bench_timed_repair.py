#!/usr/bin/env python3
"""Repaired priority orders against the same budget of random ones, on one GPU.  A budget is a number of
plans of one order: ``rmpc_timed_plan_repair_device`` with G = 16 orders and R rounds spends at most G (R + 1), and is
set against ``rmpc_timed_plan_device`` on G (R + 1) orders of ``priority_orders`` (whose first G rows are the repair's
rows), for R = 0, 1, 3, 7.  Per shape, in one session:

    plan_G16              rmpc_timed_plan_device on the G rows: the time baseline, and round 0 of every repaired row
    random_R<R>           rmpc_timed_plan_device on G (R + 1) rows
    repair_R<R>           rmpc_timed_plan_repair_device on the G rows with R rounds

each with ``ms`` (median of --reps event-timed calls, each synchronised, after one warm-up call) and, of the best
order, ``fails`` (status > 0), ``late`` (arrive > T, the failed ones among them) and ``sum_arrive``; ``clean_rows`` is the
number of rows without a late robot.  The repair also reports ``rows_improved`` (rows whose key fell below round 0's),
``rounds_run`` and ``round_best`` per row.

Shapes: the examples' store (41 x 41 cells, T = 128: the history in LDS) at B = 16, 32, 48 on the routes of
``pick_spaced_routes`` (which does not place 64 on the store's clear cells in reasonable time) and at B = 64 on distinct random free cells as
scripts/bench_timed.py draws them; a 128 x 128 store (T = 256: the history in the workspace) at B = 64, 256 on random
free cells.  sep2 = 9, lag = 1, movement 4.  The document is rewritten after every shape, so a run that is cut short
leaves the shapes it finished.

    timeout -k 10 900 python scripts/bench_timed_repair.py [--reps 5] [--out profiles/timed_repair_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

G, ROUNDS, SEP2, LAG = 16, (0, 1, 3, 7), 9, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timed_repair_bench.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import event_ms
    from robot_mpcs_amd.global_planner import pick_spaced_routes, png_values, priority_orders, shelf_map
    from robot_mpcs_amd.store import STORE as S, clear_cells

    dev, i32 = "cuda:0", torch.int32
    new = lambda *s, dt=i32: torch.empty(s, dtype=dt, device=dev)
    out = {}

    def best_of(key, best, arrive, T):
        k = int(key[int(best.item())].item())
        return dict(fails=k >> 44, late=(k >> 32) & 0xFFF, sum_arrive=k & 0xFFFFFFFF,
                    clean_rows=int((((key >> 32) & 0xFFF) == 0).sum().item()))

    for H, T, kw, fleets in ((S.H, 128, dict(aisle=S.aisle, shelf=S.shelf, gap=S.gap), ((16, True), (32, True), (48, True), (64, False))),
                             (128, 256, dict(aisle=9, shelf=4, gap=6), ((64, False), (256, False)))):
        raw = shelf_map(H, H, seed=0, **kw)
        g_raw = torch.from_numpy(png_values(raw)).to(dev)
        g_inf = torch.empty_like(g_raw)
        _lib.grid_inflate_device(g_raw, g_inf, S.cell, S.size_robot, 0.29)
        free = g_inf.cpu().numpy() < 0.8
        for B, spaced in fleets:
            rng = np.random.default_rng(0)
            if spaced:
                s, gl = pick_spaced_routes(raw > 0.5, clear_cells(raw, S.clear_cells) & free, B, rng, S.x0, S.y0, S.cell, SEP2)
            else:
                cells = rng.choice(np.flatnonzero(free.ravel()), 2 * B, replace=False).astype(np.int32)
                s, gl = cells[:B], cells[B:]
            starts, goals = torch.from_numpy(s).to(dev), torch.from_numpy(gl).to(dev)
            uniq, inv = torch.unique(goals, return_inverse=True)
            uniq, inv = uniq.to(i32).contiguous(), inv.to(i32).contiguous()
            fields, fstat = new(len(uniq), H, H, dt=torch.float64), new(len(uniq))
            _lib.grid_fields_device(g_inf, uniq, fields, fstat, 4, 0.8, 3.0)
            rows = torch.from_numpy(priority_orders(B, G * (max(ROUNDS) + 1), 0)).to(dev)
            r = {}

            def plan(n):
                orders = rows[:n].contiguous()
                work = new(_lib.timed_plan_work_bytes(H, H, T, n), dt=torch.uint8)
                paths, status, arrive, key, best = new(n, B, T + 1), new(n, B), new(n, B), new(n, dt=torch.int64), new(1)
                args = _lib.timed_plan_args(g_inf, starts, inv, fields, uniq, orders, work, paths, status, arrive, key, best,
                                            movement=4, occ_threshold=0.8, sep2=SEP2, lag=LAG)
                _lib.timed_plan_device(args)
                ms = event_ms(lambda: _lib.timed_plan_device(args), a.reps)
                return dict(ms=round(ms, 3), **best_of(key, best, arrive, T)), key.clone()

            r["plan_G16"], key0 = plan(G)
            for R in ROUNDS:
                r["random_R%d" % R], _ = plan(G * (R + 1))
                orders = rows[:G].contiguous()
                work = new(_lib.timed_plan_repair_work_bytes(H, H, T, G, B), dt=torch.uint8)
                paths, status, arrive, key, best = new(G, B, T + 1), new(G, B), new(G, B), new(G, dt=torch.int64), new(1)
                order_out, rounds_run, round_best = new(G, B), new(G), new(G)
                args = _lib.timed_repair_args(g_inf, starts, inv, fields, uniq, orders, work, paths, status, arrive, key, best,
                                              order_out, rounds_run, round_best, R, movement=4, occ_threshold=0.8, sep2=SEP2,
                                              lag=LAG)
                _lib.timed_plan_repair_device(args)
                ms = event_ms(lambda: _lib.timed_plan_repair_device(args), a.reps)
                r["repair_R%d" % R] = dict(ms=round(ms, 3), **best_of(key, best, arrive, T),
                                           rows_improved=int((key < key0).sum().item()), rounds_run=rounds_run.cpu().tolist(),
                                           round_best=round_best.cpu().tolist())
            out["%dx%d_T%d_B%d_%s" % (H, H, T, B, "spaced" if spaced else "random")] = r
            print(B, json.dumps(r), flush=True)
            with open(a.out, "w") as f:
                json.dump(dict(bench="timed_repair", device=torch.cuda.get_device_name(0), reps=a.reps, G=G, sep2=SEP2, lag=LAG,
                               cases=out), f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
