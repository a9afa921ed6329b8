"""Records tests/golden/sweep_words_parent.npz: z, exitflag, iters, kkt and obj of the batches of
tests/sweep_words_cases.py as a library returns them on an MI355X, b3 also on one wavefront (RMPC_FUSED_GRID=1, key
b3g1).  The committed file was recorded with the library of the commit before the merged sweep call stopped storing the
general rows' values and took the step lengths' operands first (SWEEPWORDS):

    RMPC_ALLOW_STALE=1 RMPC_LIB_PATH=<that commit's librmpc_hip.so> python tests/golden/make_sweep_words_parent.py OUT.npz

tests/test_gpu_sweep_words.py holds the current library to it byte for byte.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sweep_words_cases as cs  # noqa: E402
from oracle.oracle import Oracle, lib as olib  # noqa: E402
from robot_mpcs_amd._lib import Solver  # noqa: E402
from robot_mpcs_amd.scenarios import make_scenario  # noqa: E402


def main():
    scs = {key: cs.scenario(make_scenario, key) for key in cs.BATCHES}
    cold, _ = cs.oracle_warm_pair(Oracle, olib, scs["b3"])
    os.environ.pop("RMPC_FUSED_GRID", None)
    res = cs.solve_all(Solver, scs.__getitem__, cold["z"])
    os.environ["RMPC_FUSED_GRID"] = "1"   # (read when the handle is created)
    sc = scs["b3"]
    s = Solver(sc.desc, max_batch=sc.B)
    res["b3g1"] = dict(s.solve(sc.xinit, sc.x0, sc.params), last_passes=s.last_passes())
    s.close()
    out = {}
    for key, r in res.items():
        print(key, "flags", r["exitflag"].tolist(), "iterations", r["iters"].tolist(), "most passes", r["last_passes"])
        for k in cs.KEYS:
            out["%s_%s" % (key, k)] = r[k]
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
