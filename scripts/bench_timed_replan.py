#!/usr/bin/env python3
"""Time of the lifelong timed tours' entries on one GPU at the shapes of section 25's table: the
examples' store (41 x 41 cells, T = 128: the history in LDS) and a 128 x 128 store (T = 256: in the workspace),
B = 16, 64, 256 robots, G = 1, 16, 64 priority orders, K = 2 stops per robot, dwell 4, sep2 = 9, lag = 1, movement 4;
starts, stops and fields drawn as scripts/bench_timed_tours.py draws them.  Per shape, in one session:

    tours_plan_ms        rmpc_timed_tours_plan_device, whose best order's paths are what is reserved below
    reserve_ms           rmpc_timed_reserve_device of those B paths (clear = 1)
    replan_k<k>_ms       rmpc_timed_tours_replan_device of k = B/4, B/2 and B robots (the first k of a random order of
                         the robots) from layer 0 against the table of the others' paths (k = B: an empty table)
    replan_identity_ms   the same entry with no table, all active, begin 0: what the timed tours' entry computes

Times are medians of --reps event-timed calls (each synchronised), after one warm-up call.  The document is rewritten
after every shape, so a run that is cut short leaves the shapes it finished.

    timeout -k 10 900 python scripts/bench_timed_replan.py [--reps 5] [--out profiles/timed_replan_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K, DWELL = 2, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timed_replan_bench.json"))
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
            all_stops = np.stack([rng.choice(Gf, 8, replace=False) for _ in range(B)]).astype(np.int32)
            stops = torch.from_numpy(all_stops[:, :K].copy()).to(dev)
            lens = torch.full((B,), K, dtype=i32, device=dev)
            park = stops[:, K - 1].contiguous()
            robots = rng.permutation(B)
            res = new(_lib.timed_reserve_words(H, H, T), dt=torch.int64)
            for G in (1, 16, 64):
                orders = torch.from_numpy(priority_orders(B, G, 0)).to(dev)
                work = new(_lib.timed_tours_work_bytes(H, H, T, G), dt=torch.uint8)
                work2 = new(_lib.timed_replan_work_bytes(H, H, T, G), dt=torch.uint8)
                paths, status, arrive, served = new(G, B, T + 1), new(G, B), new(G, B), new(G, B)
                key, best, unserved, serve_at, clash = new(G, dt=torch.int64), new(1), new(G), new(G, B, K), new(B)
                ta = _lib.timed_tours_args(g_inf, starts, stops, lens, park, fields, picks, orders, work, paths, status, arrive,
                                           key, best, serve_at, served, unserved, dwell=DWELL, movement=4, occ_threshold=0.8,
                                           sep2=9, lag=1)
                _lib.timed_tours_plan_device(ta)
                r = dict(tours_plan_ms=round(event_ms(lambda: _lib.timed_tours_plan_device(ta), a.reps), 3))
                b = int(best.item())
                planned = paths[b].clone()
                r["best_unserved"] = int(unserved[b].item())
                _lib.timed_reserve_device(planned, res, H, H, 9, 1)
                r["reserve_ms"] = round(event_ms(lambda: _lib.timed_reserve_device(planned, res, H, H, 9, 1), a.reps), 3)
                x = _lib.timed_replan_args(work2)
                _lib.timed_tours_replan_device(ta, x)
                r["replan_identity_ms"] = round(event_ms(lambda: _lib.timed_tours_replan_device(ta, x), a.reps), 3)
                same = bool((paths[b] == planned).all().item())
                r["identity_is_the_plan"] = same
                for k in (B // 4, B // 2, B):
                    act = np.zeros(B, np.int32)
                    act[robots[:k]] = 1
                    active = torch.from_numpy(act).to(dev)
                    _lib.timed_reserve_device(planned, res, H, H, 9, 1, use=(1 - active).contiguous())
                    x = _lib.timed_replan_args(work2, res, active, None, clash)
                    _lib.timed_tours_replan_device(ta, x)
                    r[f"replan_k{k}_ms"] = round(event_ms(lambda: _lib.timed_tours_replan_device(ta, x), a.reps), 3)
                    r[f"replan_k{k}_best_unserved"] = int(unserved[int(best.item())].item())
                    r[f"replan_k{k}_clash"] = int(clash.sum().item())
                out[f"{H}x{H}_T{T}_B{B}_G{G}"] = r
                doc = dict(bench="timed_replan", device=torch.cuda.get_device_name(0), reps=a.reps, sep2=9, lag=1, movement=4,
                           K=K, dwell=DWELL, cases=out)
                with open(a.out, "w") as f:
                    f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
