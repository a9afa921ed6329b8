"""bench.py's plain run and ``--dump-outputs``: the result line of a plain run carries the headline figure and nothing
that needs runs of its own (those are ``--full``'s), and the dump is what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "legs", "extra", "cpu_baseline")


def test_dump_outputs_sample_is_seeded_and_bounded(tmp_path):
    """Within the limit every array is written whole in float64; above it each array keeps the same seeded rows, in
    index order, and the files stay within the limit."""
    import bench
    n = 1000
    idx = np.arange(n)
    arrays = {"z": idx[:, None, None] + np.zeros((n, 30, 9)), "exitflag": idx.astype(np.int32), "x": np.arange(300.0)[:, None] * np.ones(6)}
    bench.dump_outputs(str(tmp_path / "whole"), arrays)
    for k, v in arrays.items():
        got = np.load(tmp_path / "whole" / (k + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, v)
    limit = 200_000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, max_bytes=limit)
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in arrays}
    assert sum(v.nbytes for v in a.values()) <= limit
    assert all(v.dtype == np.float64 and 0 < len(v) < len(arrays[k]) for k, v in a.items())
    assert np.array_equal(a["z"][:, 0, 0], a["exitflag"])          # the same instances in both arrays of n rows
    assert np.all(np.diff(a["exitflag"]) > 0)
    for k in arrays:
        assert np.array_equal(a[k], np.load(tmp_path / "b" / (k + ".npy")))


def _bench(args, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, capture_output=True, text=True,
                       timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    """7 steps over 4 handles and 3 input sets: the last timed step is handle 2's second, on input set 1 (4 warm-up
    steps first); its dump equals a fresh handle's solve of that input set."""
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd._lib import Solver
    from robot_mpcs_amd.scenarios import make_scenario
    d = _bench(["--steps", "7", "--warmup", "2", "--streams", "4", "--input-sets", "3", "--dump-outputs", "out"], tmp_path)
    assert all(k in d for k in HEADLINE) and not any(k in d for k in FULL_ONLY)
    assert d["steps"] == 7 and d["value"] == pytest.approx(4096 * 1e3 / d["ms_per_step"], rel=1e-9)
    got = {k: np.load(tmp_path / "out" / (k + ".npy")) for k in ("z", "exitflag", "iters", "kkt", "obj")}
    assert all(v.dtype == np.float64 and len(v) == 4096 for v in got.values())
    sc = make_scenario("cfg2", B=4096, seed=1000 + 17 * 1)
    s = Solver(sc.desc, max_batch=4096, device=0)
    ref = s.solve(sc.xinit, sc.x0, sc.params)
    s.close()
    assert np.array_equal(got["exitflag"], ref["exitflag"]) and np.array_equal(got["iters"], ref["iters"])
    assert np.abs(got["z"] - ref["z"]).max() <= 1e-9 * max(1.0, float(np.abs(ref["z"]).max()))


@pytest.mark.gpu
def test_plain_cfg5_run_dumps_every_block(tmp_path):
    d = _bench(["--config", "cfg5", "--steps", "2", "--warmup", "1", "--dump-outputs", "out"], tmp_path)
    assert all(k in d for k in HEADLINE) and d["steps"] == 2
    for name, B in (("cfg2", 4096), ("cfg3", 3072), ("cfg4", 1024)):
        for k in ("z", "exitflag", "iters", "kkt", "obj", "x"):
            v = np.load(tmp_path / "out" / ("%s_%s.npy" % (name, k)))
            assert v.dtype == np.float64 and len(v) == B
