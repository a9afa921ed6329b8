#!/usr/bin/env python3
"""Development aid: solve seeded batches with the library named by RMPC_LIB_PATH and dump the raw results, so that
two builds can be compared bit for bit (tests/tools/ab_compare.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from robot_mpcs_amd._lib import Solver  # noqa: E402
from robot_mpcs_amd.scenarios import make_scenario  # noqa: E402

out = {}
NOF = {"RMPC_NO_FUSED": "1"}
LANE = {"RMPC_NO_FUSED": "1", "RMPC_RIC_LANE": "2"}
TWO = {"RMPC_ARM_TWO_PARTS": "1"}
# (name, batch, seed, scenario keywords, switches read at rmpc_create): between them every path of the table in
# tests/test_gpu_newton_step.py
cases = [("cfg1", 1, 0, {}, {}), ("cfg2", 700, 1, {}, {}), ("cfg3", 700, 2, {}, {}), ("cfg4", 300, 3, {}, {}),
         ("boxer", 130, 4, {}, {}), ("wc_point", 200, 5, {}, {}), ("wc_boxer", 200, 6, {}, {}),
         ("wc_boxer_slack", 200, 7, {}, {}), ("wc_panda", 64, 8, {}, {}), ("cfg2", 4096, 9, {}, {}),
         ("cfg2", 300, 10, dict(slack=True), {}), ("chain2", 300, 11, {}, {}), ("chain4", 100, 12, {}, {}),
         ("chain5", 100, 13, {}, {}), ("chain6", 100, 14, {}, {}), ("chain8", 64, 15, {}, {}),
         ("cfg4", 64, 16, {}, TWO), ("cfg2", 200, 17, {}, NOF), ("cfg2", 200, 18, dict(slack=True), NOF),
         ("cfg4", 64, 19, {}, NOF), ("boxer", 64, 20, {}, NOF), ("cfg2", 200, 21, {}, LANE), ("chain2", 200, 22, {}, LANE)]
for name, B, seed, kw, env in cases:
    sc = make_scenario(name, B=B, seed=seed, **kw)
    os.environ.update(env)
    s = Solver(sc.desc, max_batch=B)
    for k in env:
        del os.environ[k]
    r = s.solve(sc.xinit, sc.x0, sc.params)
    s.close()
    tag = "".join("_" + k for k in sorted(kw)) + "".join("_" + k[5:] for k in sorted(env))
    for k in ("z", "exitflag", "iters", "kkt", "obj"):
        out[f"{name}_{B}{tag}_{k}"] = r[k]
    print(name, B, tag, "iters mean", r["iters"].mean(), "flags", np.unique(r["exitflag"], return_counts=True), flush=True)
np.savez(sys.argv[1], **out)
