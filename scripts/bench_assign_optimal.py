#!/usr/bin/env python3
"""Event-timed medians of the minimum-cost assignment on the device: the whole call
(rmpc_assign_optimal_device: memset, quantise pre-pass, solver), the pre-pass alone measured as the call on a matrix
whose search is trivial (all costs distinct per column: m steps), and rmpc_assign_greedy_device beside it at the same
shapes, with G = 1 and G = 16 problems per call (greedy: G calls), the steps of the search and microseconds per step.

    python scripts/bench_assign_optimal.py [--reps 20]

Prints one JSON line per (kind, B, T, G).  No time is gated.
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

CASES = [("grid", 16, 24), ("grid", 64, 64), ("grid", 256, 256), ("grid", 1024, 1024), ("grid", 4096, 256),
         ("const", 256, 256)]


def diagonal_costs(B, T):
    """every robot's cheapest target is its own (b mod T): the search takes min(B, T) steps, what is left is the pre-pass,
    the launches and the report"""
    c = np.full((B, T), 50.0)
    c[np.arange(B), np.arange(B) % T] = 1.0
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from assign_optimal_cases import make_costs
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import event_ms
    dev = "cuda:0"
    for kind, B, T in CASES:
        one = make_costs(kind, B, T)
        for G in (1, 16):
            cost = torch.from_numpy(np.stack([one] * G) if kind == "const" else
                                    np.stack([make_costs(kind, B, T, seed=s) for s in range(G)])).to(dev)
            easy = torch.from_numpy(np.stack([diagonal_costs(B, T)] * G)).to(dev)
            assign = torch.empty((G, B), dtype=torch.int32, device=dev)
            total = torch.empty(G, dtype=torch.int64, device=dev)
            count, steps = torch.empty(G, dtype=torch.int32, device=dev), torch.empty(G, dtype=torch.int32, device=dev)
            work = torch.empty(_lib.assign_optimal_work_bytes(G, B, T), dtype=torch.uint8, device=dev)
            call = lambda c: _lib.assign_optimal_device(c, assign, 1024.0, total, count, steps, work)
            ms = event_ms(lambda: call(cost), a.reps)
            n_steps = steps.cpu().numpy().copy()
            ms_easy = event_ms(lambda: call(easy), a.reps)
            easy_steps = int(steps.max().item())

            def greedy():
                for i in range(G):
                    _lib.assign_greedy_device(cost[i], assign[i])
            ms_greedy = event_ms(greedy, a.reps)
            print(json.dumps(dict(kind=kind, B=B, T=T, G=G, optimal_ms=round(ms, 4), steps_max=int(n_steps.max()),
                                  steps_mean=float(n_steps.mean()),
                                  us_per_step=round(1e3 * (ms - ms_easy) / max(int(n_steps.max()) - easy_steps, 1), 4),
                                  trivial_search_ms=round(ms_easy, 4), trivial_search_steps=easy_steps,
                                  greedy_ms=round(ms_greedy, 4), reps=a.reps)), flush=True)


if __name__ == "__main__":
    main()
