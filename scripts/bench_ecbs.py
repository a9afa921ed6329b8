#!/usr/bin/env python3
"""Focal conflict-based search over the timed routes on one GPU: what a round costs beside a round of
rmpc_cbs_device under the same protocol in the same session, and what the search finds on the store.  Per map:

    round_E<E>     for each of the two entries (``ecbs`` at w = 21/20, ``cbs``): a search on 8 robots is grown with rounds
                   of E nodes until a round takes E of them or eight calls have passed; then ``--reps`` resumed calls of
                   ROUNDS rounds each are event-timed: ``ms_per_round`` (median call / ROUNDS), ``taken_per_round`` and
                   ``children_per_round`` over those calls (a batch that FOCAL or the open list cannot fill says so
                   here); a search that stops before that reports its outcome beside the figures
    store          (the store only) 4, 8, 16 and 32 robots, w in 1, 21/20, 11/10, 6/5, seeds 0 to 3, one node per round,
                   ROUNDS_STORE rounds and NODES_STORE nodes: outcome, expanded, cost, bound, lb and nconf of the reported
                   node, ms of the call; beside it the sum of arrivals of the best of 16 orders with 3 repair rounds

Maps: the examples' store (41 x 41 cells, T = 128: history and cost rows in LDS) and a 128 x 128 store (T = 256: both in
the workspace).  sep2 = 9, lag = 1, movement 4.  The document is rewritten after every entry.

    timeout -k 10 900 python scripts/bench_ecbs.py [--reps 5] [--out profiles/ecbs_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEP2, LAG, ROUNDS, BATCHES = 9, 1, 4, (1, 16, 64)
W_ROUND = (21, 20)          # at 11/10 the 8-robot search is solved after 4 expansions: no rounds left to time
WEIGHTS = ((1, 1), (21, 20), (11, 10), (6, 5))
FLEETS, SEEDS, ROUNDS_STORE, NODES_STORE = (4, 8, 16, 32), (0, 1, 2, 3), 1024, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecbs_bench.json"))
    ap.add_argument("--skip-store", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import event_ms
    from robot_mpcs_amd.global_planner import (BoundedTimedRoutes, TimedRoutes, pick_spaced_routes, png_values, shelf_map)
    from robot_mpcs_amd.store import STORE as S, clear_cells, store_map

    dev, i32 = "cuda:0", torch.int32
    new = lambda *s, dt=i32: torch.empty(s, dtype=dt, device=dev)
    out = {}

    def write():
        with open(a.out, "w") as f:
            json.dump(dict(bench="ecbs", device=torch.cuda.get_device_name(0), reps=a.reps, sep2=SEP2, lag=LAG,
                           rounds_per_call=ROUNDS, w_round=list(W_ROUND), cases=out), f, indent=1)
            f.write("\n")

    def inflate(raw):
        g_raw = torch.from_numpy(png_values(raw)).to(dev)
        g_inf = torch.empty_like(g_raw)
        _lib.grid_inflate_device(g_raw, g_inf, S.cell, S.size_robot, 0.29)
        return g_inf, clear_cells(raw, S.clear_cells) & (g_inf.cpu().numpy() < 0.8)

    for name, H, T, FLEET, kw in (("store", S.H, 128, 8, dict(aisle=S.aisle, shelf=S.shelf, gap=S.gap)),
                                  ("128x128", 128, 256, 8, dict(aisle=9, shelf=4, gap=6))):
        raw = shelf_map(H, H, seed=0, **kw)
        g_inf, ok = inflate(raw)
        r = out[name] = {}
        s, gl = pick_spaced_routes(raw > 0.5, ok, FLEET, np.random.default_rng(0), S.x0, S.y0, S.cell, SEP2)
        starts, goals = torch.from_numpy(s).to(dev), torch.from_numpy(gl).to(dev)
        uniq, inv = torch.unique(goals, return_inverse=True)
        uniq, inv = uniq.to(i32).contiguous(), inv.to(i32).contiguous()
        fields, fstat = new(len(uniq), H, H, dt=torch.float64), new(len(uniq))
        _lib.grid_fields_device(g_inf, uniq, fields, fstat, 4, 0.8, 3.0)

        def search(entry, nodes, E):
            focal = entry == "ecbs"
            nbytes = (_lib.ecbs_work_bytes if focal else _lib.cbs_work_bytes)(H, H, T, FLEET, nodes, E)
            work = new(nbytes, dt=torch.uint8)
            paths, status, arrive, info = new(FLEET, T + 1), new(FLEET), new(FLEET), new(_lib.ECBS_INFO)
            common = dict(movement=4, occ_threshold=0.8, sep2=SEP2, lag=LAG)
            if focal:
                call = lambda rounds, resume: _lib.ecbs_device(_lib.ecbs_args(
                    g_inf, starts, inv, fields, uniq, work, paths, status, arrive, info, nodes, E, rounds, w=W_ROUND,
                    resume=resume, **common))
            else:
                call = lambda rounds, resume: _lib.cbs_device(_lib.cbs_args(
                    g_inf, starts, inv, fields, uniq, work, paths, status, arrive, info, nodes, E, rounds, resume=resume,
                    **common))
            return call, info, nbytes

        for E in BATCHES:
            row = r["round_E%d" % E] = {}
            for entry in ("ecbs", "cbs"):
                nodes = min(_lib.CBS_MAX_NODES, 2 * E * ROUNDS * (a.reps + 12) + 4096)
                call, info, nbytes = search(entry, nodes, E)
                call(32, False)
                for _ in range(8):                         # until a round of E nodes is a full one
                    before = int(info[_lib.CBS_EXPANDED].item())
                    call(ROUNDS, True)
                    if int(info[_lib.CBS_EXPANDED].item()) - before == E * ROUNDS:
                        break
                before = info.cpu().tolist()
                ms = event_ms(lambda: call(ROUNDS, True), a.reps)
                after = info.cpu().tolist()
                n = (after[_lib.CBS_ROUNDS_RUN] - before[_lib.CBS_ROUNDS_RUN]) or 1
                made = after[_lib.CBS_CREATED] - before[_lib.CBS_CREATED]
                row[entry] = dict(ms_per_round=round(ms / ROUNDS, 4), outcome=after[_lib.CBS_OUTCOME],
                                  taken_per_round=round((after[_lib.CBS_EXPANDED] - before[_lib.CBS_EXPANDED]) / n, 2),
                                  children_per_round=round(made / n, 2), pool=nodes, work_mb=round(nbytes / 2 ** 20, 1))
                print(name, E, entry, json.dumps(row[entry]), flush=True)
                write()

    if not a.skip_store:
        H, T = S.H, 128
        rows = out["store"]["fleets"] = []
        for seed in SEEDS:
            raw = store_map(seed)
            g_inf, ok = inflate(raw)
            for B in FLEETS:
                try:
                    s, gl = pick_spaced_routes(raw > 0.5, ok, B, np.random.default_rng(seed), S.x0, S.y0, S.cell, SEP2)
                except Exception as e:                      # the store has no room for that many spaced routes
                    rows.append(dict(seed=seed, B=B, error=str(e)[:80]))
                    continue
                starts, goals = torch.from_numpy(s).to(dev), torch.from_numpy(gl).to(dev)
                rep = TimedRoutes(g_inf, 4, 0.8, T, SEP2, lag=LAG, orders=16, seed=seed, device=dev, repair=3)
                _, status, arrive, best = rep.plan(starts, goals)
                b = int(best.item())
                prio = dict(prioritised_sum=int(arrive[b].sum().item()), prioritised_failures=int((status[b] > 0).sum().item()))
                for w in WEIGHTS:
                    btr = BoundedTimedRoutes(g_inf, 4, 0.8, T, SEP2, w=w, lag=LAG, nodes=NODES_STORE, expand=1,
                                             rounds=ROUNDS_STORE, device=dev)
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()                             # one call, fields included: a search is not repeated here
                    btr.plan(starts, goals)
                    t1.record()
                    t1.synchronize()
                    ms = t0.elapsed_time(t1)
                    found = dict(zip((n.lower() for n in _lib.ECBS_INFO_NAMES), btr.info.cpu().tolist()))
                    rows.append(dict(seed=seed, B=B, w=list(w), **found, ms=round(ms, 2), **prio))
                    print(json.dumps(rows[-1]), flush=True)
                    write()


if __name__ == "__main__":
    main()
