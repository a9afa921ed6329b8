#!/usr/bin/env python3
"""The closed loop of examples/fleet_store_corridor.py (256 robots, seed 0, 1200 control steps; include/rmpc_corridor.h,
DESIGN.md 29) with corridors and without them (``--no-corridor``, the baseline: the same model, dummy planes) at the
waypoint thresholds 0.6 m (the example's default), 0.9 m and 1.3 m (the reference's, what fleet_global_route.py
takes), and at the default with the separating planes against 4 neighbours behind the corridor's slots, in one
session: arrivals and arrival p50 / p90 / max, failed and flag-0 solves and the share of solves that did not converge,
the failed solves that had a seed closer than r_body to a face of its rectangle, the share of seeds without a corridor,
the least clearance over all robot-steps, over the converged ones and over the converged ones whose every stage had a
corridor with the seed r_body inside, the highest speed, ms per control step and per ``MapCorridors.step``.

    timeout -k 10 600 python scripts/sweep_corridor_loop.py [--steps 1200] [--out profiles/corridor_loop.json]

Writes the JSON to --out and prints one line per run.  Nothing is gated.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

RUNS = [dict(threshold=t, corridor=c) for t in (0.6, 0.9, 1.3) for c in (False, True)]
RUNS += [dict(threshold=0.6, corridor=c, neighbours=4) for c in (False, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corridor_loop.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from example_loader import load_example
    from robot_mpcs_amd import _lib
    ex = load_example("fleet_store_corridor")
    rows = []
    for kw in RUNS:
        rows.append(ex.run(B=256, steps=a.steps, seed=0, **kw))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(sweep="corridor_loop", device=torch.cuda.get_device_name(0), robots=256, seed=0, steps=a.steps,
               source_hash=_lib.source_hash(), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
