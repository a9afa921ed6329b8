#!/usr/bin/env python3
"""The closed loop of examples/fleet_global_route.py (256 robots, seed 0, 1200 control steps) under the waypoint
follower at thresholds 1.3 m and 0.7 m and under the visible follower (include/rmpc_any_angle.h) at
look-aheads 1.3, 1.75 and 2.2 m (the reference's threshold, that plus one cell, plus two cells), reach 16, seeing on the
enlarged map and on the store as it is, and at the middle look-ahead with reach 4 and 64, in one session: least and p10 clearance, arrival p50 / p90 / max, failed
solves, blocked robot-steps, ms per control step.

    timeout -k 10 600 python scripts/sweep_visible_follower.py [--steps 1200] [--out profiles/any_angle_sweep.json]

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

RUNS = [dict(follower="waypoint", threshold=1.3), dict(follower="waypoint", threshold=0.7)]
RUNS += [dict(follower="visible", look_ahead=v, reach=16, sight=m) for m in ("enlarged", "raw") for v in (1.3, 1.75, 2.2)]
RUNS += [dict(follower="visible", look_ahead=1.75, reach=r, sight="raw") for r in (4, 64)]
KEYS = ("routes", "failed_solves", "arrivals", "arrival_step_p50", "arrival_step_p90", "arrival_step_max", "min_clearance_m",
        "clearance_p10", "touching", "blocked_robot_steps", "ms_per_step", "route_cells_dense", "route_cells_any_angle",
        "route_m_dense", "route_m_any_angle")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "any_angle_sweep.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from example_loader import load_example
    from robot_mpcs_amd import _lib
    ex = load_example("fleet_global_route")
    rows = []
    for kw in RUNS:
        r = ex.run(B=256, steps=a.steps, seed=0, **kw)
        rows.append(dict(kw, **{k: r[k] for k in KEYS}))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(sweep="visible_follower", device=torch.cuda.get_device_name(0), robots=256, seed=0, steps=a.steps,
               source_hash=_lib.source_hash(), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
