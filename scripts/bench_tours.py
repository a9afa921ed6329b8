#!/usr/bin/env python3
"""Event-timed medians of the tours on the device: the whole call (rmpc_tours_device: quantise pre-pass
and the workgroup per problem that builds and improves), in both modes, with G = 1 and G = 16 problems per call, on
octile distances between random cells ("grid" of tests/tours_cases.py), together with the build steps and the rounds the
improvement took, and the same call with max_rounds = 0 (the build alone).

    python scripts/bench_tours.py [--reps 5] [--json profiles/tours_bench.json]

Prints one JSON line per (B, T, K, G, mode) and writes them all to --json.  No time is gated.
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

CASES = [(16, 24, 2), (64, 256, 8), (1, 256, 256), (256, 1024, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "tours_bench.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from tours_cases import make_problem
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import event_ms
    dev = "cuda:0"
    lines = []
    for B, T, K in CASES:
        for G in (1, 16):
            probs = [make_problem("grid", B, T, seed=s) for s in range(G)]
            s = torch.from_numpy(np.stack([p[0] for p in probs])).to(dev)
            d = torch.from_numpy(np.stack([p[1] for p in probs])).to(dev)
            tours = torch.empty((G, B, K), dtype=torch.int32, device=dev)
            lens = torch.empty((G, B), dtype=torch.int32, device=dev)
            cost = torch.empty((G, B), dtype=torch.int64, device=dev)
            count, steps, rounds = (torch.empty(G, dtype=torch.int32, device=dev) for _ in range(3))
            total, span = (torch.empty(G, dtype=torch.int64, device=dev) for _ in range(2))
            work = torch.empty(_lib.tours_work_bytes(G, B, T), dtype=torch.uint8, device=dev)
            for mode in ("sum", "span"):
                call = lambda cap: _lib.tours_device(s, d, tours, lens, cost, mode, 1024.0, cap, None, count, total, span,
                                                     steps, rounds, work)
                ms_build = event_ms(lambda: call(0), a.reps)
                built = (total.cpu().numpy().copy(), span.cpu().numpy().copy())
                ms = event_ms(lambda: call(1 << 30), a.reps)
                r, n = rounds.cpu().numpy(), steps.cpu().numpy()
                lines.append(dict(B=B, T=T, K=K, G=G, mode=mode, ms=round(ms, 4), build_only_ms=round(ms_build, 4),
                                  build_steps=int(n.max()), rounds_max=int(r.max()), rounds_mean=float(r.mean()),
                                  us_per_build_step=round(1e3 * ms_build / max(int(n.max()), 1), 3),
                                  us_per_round=round(1e3 * (ms - ms_build) / max(int(r.max()), 1), 3),
                                  count_min=int(count.min().item()), total_q_built=int(built[0][0]),
                                  total_q=int(total[0].item()), span_q_built=int(built[1][0]), span_q=int(span[0].item()),
                                  reps=a.reps, library_source_hash=_lib.load_library().rmpc_source_hash().decode()))
                print(json.dumps(lines[-1]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
