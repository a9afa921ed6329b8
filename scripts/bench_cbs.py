#!/usr/bin/env python3
"""Conflict-based search over the timed routes on one GPU: what a round costs, what rounds behind a
finished search cost, and what the search finds on the store.  Per map, in one session:

    round_E<E>     a search on 8 robots is grown with rounds of E nodes until a round takes E of them (a search that is
                   solved before that reports its outcome and no figures); then ``--reps`` resumed calls of ROUNDS
                   rounds each are event-timed: ``ms_per_round`` (median call / ROUNDS),
                   ``taken_per_round`` and ``children_per_round`` over those calls (a batch that the open list cannot
                   fill says so here), ``nodes_per_s`` = children made per second
    idle           ``ms_per_idle_round``: a one-robot search is solved at its root; the median call of IDLE rounds
                   behind it, less the call of no rounds, over IDLE
    plan_per_robot ``k_timed_plan`` on one order of the same robots: ms per planned robot, the figure a child is held
                   against
    store_B<B>     (the store only) the search under the class defaults at 4, 8 and 16 robots: outcome, expanded, cost,
                   bound, ms of the call; beside it the sum of arrivals of the best of 16 orders with 3 repair rounds

Maps: the examples' store (41 x 41 cells, T = 128: the history in LDS) and a 128 x 128 store (T = 256: the history in the
workspace).  sep2 = 9, lag = 1, movement 4.  The document is rewritten after every entry.

    timeout -k 10 900 python scripts/bench_cbs.py [--reps 5] [--out profiles/cbs_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEP2, LAG, ROUNDS, IDLE, BATCHES = 9, 1, 4, 1024, (1, 16, 64, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cbs_bench.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import event_ms
    from robot_mpcs_amd.global_planner import (OptimalTimedRoutes, TimedRoutes, pick_spaced_routes, png_values, shelf_map)
    from robot_mpcs_amd.store import STORE as S, clear_cells

    dev, i32 = "cuda:0", torch.int32
    new = lambda *s, dt=i32: torch.empty(s, dtype=dt, device=dev)
    out = {}

    def write():
        with open(a.out, "w") as f:
            json.dump(dict(bench="cbs", device=torch.cuda.get_device_name(0), reps=a.reps, sep2=SEP2, lag=LAG,
                           rounds_per_call=ROUNDS, idle_rounds=IDLE, cases=out), f, indent=1)
            f.write("\n")

    for name, H, T, FLEET, kw in (("store", S.H, 128, 8, dict(aisle=S.aisle, shelf=S.shelf, gap=S.gap)),
                                  ("128x128", 128, 256, 8, dict(aisle=9, shelf=4, gap=6))):
        raw = shelf_map(H, H, seed=0, **kw)
        g_raw = torch.from_numpy(png_values(raw)).to(dev)
        g_inf = torch.empty_like(g_raw)
        _lib.grid_inflate_device(g_raw, g_inf, S.cell, S.size_robot, 0.29)
        ok = clear_cells(raw, S.clear_cells) & (g_inf.cpu().numpy() < 0.8)
        r = out[name] = {}

        def routes(B):
            s, gl = pick_spaced_routes(raw > 0.5, ok, B, np.random.default_rng(0), S.x0, S.y0, S.cell, SEP2)
            starts, goals = torch.from_numpy(s).to(dev), torch.from_numpy(gl).to(dev)
            uniq, inv = torch.unique(goals, return_inverse=True)
            uniq, inv = uniq.to(i32).contiguous(), inv.to(i32).contiguous()
            fields, fstat = new(len(uniq), H, H, dt=torch.float64), new(len(uniq))
            _lib.grid_fields_device(g_inf, uniq, fields, fstat, 4, 0.8, 3.0)
            return starts, goals, inv, fields, uniq

        def search(B, inputs, nodes, E):
            starts, _, inv, fields, uniq = inputs
            work = new(_lib.cbs_work_bytes(H, H, T, B, nodes, E), dt=torch.uint8)
            paths, status, arrive, info = new(B, T + 1), new(B), new(B), new(_lib.CBS_INFO)
            call = lambda rounds, resume: _lib.cbs_device(_lib.cbs_args(
                g_inf, starts, inv, fields, uniq, work, paths, status, arrive, info, nodes, E, rounds, resume=resume,
                movement=4, occ_threshold=0.8, sep2=SEP2, lag=LAG))
            return call, info

        inputs = routes(FLEET)
        for E in BATCHES:
            nodes = min(_lib.CBS_MAX_NODES, 2 * E * ROUNDS * (a.reps + 12) + 4096)
            call, info = search(FLEET, inputs, nodes, E)
            call(32, False)
            grown = 0
            for _ in range(8):                         # until a round of E nodes is a full one
                before = int(info[_lib.CBS_EXPANDED].item())
                call(ROUNDS, True)
                grown = int(info[_lib.CBS_EXPANDED].item()) - before
                if grown == E * ROUNDS:
                    break
            before = info.cpu().tolist()
            ms = event_ms(lambda: call(ROUNDS, True), a.reps)
            after = info.cpu().tolist()
            n = (after[_lib.CBS_ROUNDS_RUN] - before[_lib.CBS_ROUNDS_RUN]) or 1
            made = after[_lib.CBS_CREATED] - before[_lib.CBS_CREATED]
            r["round_E%d" % E] = dict(ms_per_round=round(ms / ROUNDS, 4), outcome=after[_lib.CBS_OUTCOME],
                                      taken_per_round=round((after[_lib.CBS_EXPANDED] - before[_lib.CBS_EXPANDED]) / n, 2),
                                      children_per_round=round(made / n, 2),
                                      nodes_per_s=round(made / n / (ms / ROUNDS) * 1e3, 1), pool=nodes)
            print(name, E, json.dumps(r["round_E%d" % E]), flush=True)
            write()

        one = routes(1)
        call, info = search(1, one, 16, 16)
        call(1, False)
        none = event_ms(lambda: call(0, True), a.reps)
        idle = event_ms(lambda: call(IDLE, True), a.reps)
        r["idle"] = dict(ms_per_idle_round=round((idle - none) / IDLE, 5), ms_call_of_no_rounds=round(none, 4),
                         outcome=int(info[_lib.CBS_OUTCOME].item()))
        starts, goals = inputs[0], inputs[1]
        tr = TimedRoutes(g_inf, 4, 0.8, T, SEP2, lag=LAG, orders=1, device=dev)
        r["plan_per_robot"] = dict(ms=round(event_ms(lambda: tr.plan(starts, goals), a.reps) / FLEET, 4), B=FLEET)
        print(name, json.dumps(r["idle"]), json.dumps(r["plan_per_robot"]), flush=True)
        write()

        if name == "store":
            for B in (4, 8, 16):
                starts, goals = routes(B)[:2]
                otr = OptimalTimedRoutes(g_inf, 4, 0.8, T, SEP2, lag=LAG, device=dev)
                otr.plan(starts, goals)
                ms = event_ms(lambda: otr.plan(starts, goals), 3)
                found = dict(zip((n.lower() for n in _lib.CBS_INFO_NAMES), otr.info.cpu().tolist()))
                rep = TimedRoutes(g_inf, 4, 0.8, T, SEP2, lag=LAG, orders=16, seed=0, device=dev, repair=3)
                _, status, arrive, best = rep.plan(starts, goals)
                b = int(best.item())
                r["store_B%d" % B] = dict(found, ms=round(ms, 3), nodes=otr.nodes, expand=otr.expand, rounds=otr.rounds,
                                          prioritised_sum=int(arrive[b].sum().item()),
                                          prioritised_failures=int((status[b] > 0).sum().item()))
                print(name, B, json.dumps(r["store_B%d" % B]), flush=True)
                write()


if __name__ == "__main__":
    main()
