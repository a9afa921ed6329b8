#!/usr/bin/env python3
"""Time of wide-window localisation on one GPU, in one process on the examples' store (41 x 41 cells at
sub 8) with R = 64 rays at B = 64, 256 and 4096 robots; the ranges are the device's own scan at the true poses:

  (a) ``rmpc_scan_match_device`` at 31 x 31 x 31 (0.02 m, 0.005 rad), priors within 0.25 m and 0.06 rad: the brute force
      at its largest lattice, the comparator;
  (b) ``rmpc_scan_search_device`` over that same lattice and those priors;
  (c) ``rmpc_scan_search_device`` at 81 x 81 x 41 (0.0375 m, 0.02 rad), priors within 1.5 m and 0.4 rad: nine times the
      candidates.

Each is the entry alone on points projected once (``*_ms``) and the class's ``step`` with the projection
(``*_step_ms``).  With them: the mean and the maximum of leaves / K of the searches, whether (b) returned (a)'s poses,
and the time of ``ScanSearcher.set_map`` (the pyramid, one launch per level).

Times are medians of --reps event-timed calls (each synchronised), after one warm-up call.

    timeout -k 10 300 python scripts/bench_scan_search.py [--reps 20] [--top-log2 3] [--out FILE]

Prints one JSON line, and writes it to --out when given.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--top-log2", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import event_ms
    from robot_mpcs_amd.store import STORE as S, clear_cells, store_map
    from robot_mpcs_amd.utils.lidar import boxes_from_grid
    from robot_mpcs_amd.utils.localization import ScanMatcher, ScanSearcher

    dev = "cuda:0"
    rng = np.random.default_rng(0)
    rays, max_range, offset, height = 64, 10.0, (S.ee_offset, 0.0), 0.02
    raw = store_map(0)
    grid = torch.from_numpy(raw.astype(np.float64)).to(dev)
    boxes = torch.from_numpy(boxes_from_grid(raw, S.x0, S.y0, S.cell)).to(dev)
    ok = np.flatnonzero(clear_cells(raw, 2).ravel())
    brute, wide = dict(nxy=15, step_xy=0.02, nth=15, step_th=0.005), dict(nxy=40, step_xy=0.0375, nth=20, step_th=0.02)
    out = {}
    for B in (64, 256, 4096):
        cells = rng.choice(ok, B)
        true = np.zeros((B, 8))
        true[:, 0] = S.x0 + (cells % S.W) * S.cell + rng.uniform(-0.2, 0.2, B)
        true[:, 1] = S.y0 + (cells // S.W) * S.cell + rng.uniform(-0.2, 0.2, B)
        true[:, 2] = rng.uniform(-math.pi, math.pi, B)
        near, far = true.copy(), true.copy()
        near[:, :3] += rng.uniform(-1, 1, (B, 3)) * [0.25, 0.25, 0.06]
        far[:, :3] += rng.uniform(-1, 1, (B, 3)) * [1.5, 1.5, 0.4]
        d_true, d_near, d_far = (torch.from_numpy(v).to(dev) for v in (true, near, far))
        points = torch.zeros((B, rays, 3), dtype=torch.float64, device=dev)
        ranges = torch.zeros((B, rays), dtype=torch.float64, device=dev)
        _lib.lidar_scan_device(d_true, points, boxes, None, max_range=max_range, offset=offset, height=height, ranges=ranges)
        m = ScanMatcher(B, S.H, S.W, S.x0, S.y0, S.cell, rays, max_range, offset, height, -math.pi, math.pi, device=dev, **brute)
        m.set_map(grid, 0.5)
        r = {}

        def entry(obj, prior, search):
            """the entry alone, on the points of one projection at the prior"""
            obj.step(prior, ranges)
            src = obj.matcher if search else obj
            args = _lib.scan_match_args(prior, obj.points, ranges, src.d2, obj.rot, obj.pose_out, obj.best, obj.score, S.H,
                                        S.W, src.sub, src.cap, S.x0, S.y0, S.cell, obj.nxy, obj.step_xy, obj.nth,
                                        obj.step_th, max_range, src.min_hits, obj.score0, obj.used)
            if not search:
                return lambda: _lib.scan_match_device(args, B)
            sargs = _lib.scan_search_args(args, obj.pyr, obj.top_log2, obj.work, leaves=obj.leaves)
            return lambda: _lib.scan_search_device(sargs, B)

        r["a_match_ms"] = round(event_ms(entry(m, d_near, False), a.reps), 4)
        r["a_match_step_ms"] = round(event_ms(lambda: m.step(d_near, ranges), a.reps), 4)
        a_pose, a_best = m.pose_out.clone(), m.best.clone()
        for tag, lat, prior in (("b", brute, d_near), ("c", wide, d_far)):
            s = ScanSearcher(m, top_log2=a.top_log2, **lat)
            r[tag + "_set_map_ms"] = round(event_ms(lambda: s.set_map(), a.reps), 4)
            r[tag + "_search_ms"] = round(event_ms(entry(s, prior, True), a.reps), 4)
            r[tag + "_search_step_ms"] = round(event_ms(lambda: s.step(prior, ranges), a.reps), 4)
            K = (2 * lat["nxy"] + 1) ** 2 * (2 * lat["nth"] + 1)
            share = s.leaves[s.best >= 0].double() / K
            err = (s.pose_out[:, :2] - d_true[:, :2]).norm(dim=1)
            r.update({tag + "_levels": s.levels, tag + "_matched": int((s.best >= 0).sum().item()),
                      tag + "_leaf_share_mean": round(float(share.mean().item()), 6),
                      tag + "_leaf_share_max": round(float(share.max().item()), 6),
                      tag + "_pos_err_median_m": round(float(err.median().item()), 4),
                      tag + "_within_0.1125_m": int((err <= 0.1125).sum().item())})
            if tag == "b":
                r["b_equals_a"] = bool(torch.equal(s.pose_out, a_pose) and torch.equal(s.best, a_best))
            del s
        r["c_below_a"] = bool(r["c_search_ms"] < r["a_match_ms"])
        out[f"B{B}"] = r
    line = json.dumps(dict(bench="scan_search", device=torch.cuda.get_device_name(0), reps=a.reps, rays=rays, sub=8, cap=256,
                           top_log2=a.top_log2, cases=out))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
