"""The backward stage of the point robot's recursion in k_fused (ric_point_robot) exchanges Quu between lanes by DPP row
broadcast (row_newbcast), not through LDS: the n x n block grid sits in quads of the first 16-lane row of the instance
(lane 4 i + j), every lane of that row takes the lower triangle of Quu straight from the registers of the lanes that
formed it, and the factorisation runs ahead of the LDS round trip of [Qux | qu].  The second row of a half holds no
Quu; the flag of the factorisation is the first row's, handed to all lanes once behind the loop.  No floating-point
operation changes, so every case is held to the oracle at the bars of tests/test_gpu_parity.py (equal flags, iteration
counts, plans to 1e-6 relative, objective to 1e-9), at the smallest shapes that take each path:

  horizons 2, 3, 4, 29, 30, 31, 32, B = 3   both ends of the 32 slots, the rollout's first stage alone / an odd stage
                                            behind the pairs / pairs only; B = 3: one wavefront with both halves busy,
                                            one with an idle half
  cfg1, B = 1                               the call is entered by one half only: a row move reads the reader's own row
  chain2, B = 4                             n = 2: other broadcast lanes (0, 4, 5), other idle lanes of the quads
  cfg2, B = 5, RMPC_NO_SPEC=1, fresh process   the runtime tables (the variable is read when a handle is created)
  cfg2, B = 5, N = 3, after poison_lds()    the flag's word, the zeros and the dummy words are the call's own; what the
                                            lanes without a valid Quu compute never reaches a live word
  cfg2, B = 8, seed 6                       an instance whose curvature step is turned down (see the test): the branches
                                            behind the recursion's flag run, on a flag all lanes of the half agree on
  cfg4, B = 2                               dpp_sum8 (the arms) shares the DPP helpers
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from gpu_support import check_plan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    import __graft_entry__ as g
    g.build()
    from oracle.oracle import Oracle
    from robot_mpcs_amd._lib import Solver
    from robot_mpcs_amd.scenarios import make_scenario
    return dict(Oracle=Oracle, Solver=Solver, make_scenario=make_scenario)


def _compare(name, kw, B, gpu, cpu, nxs):
    print("%s %s B=%d: flags %s, iterations gpu %s oracle %s, max plan error %.3e, max objective error %.3e" % (
        name, kw, B, gpu["exitflag"].tolist(), gpu["iters"].tolist(), cpu["iters"].tolist(),
        np.abs(gpu["z"] - cpu["z"]).max(), np.abs(gpu["obj"] - cpu["obj"]).max()))
    check_plan(gpu, cpu, nxs)
    np.testing.assert_allclose(gpu["obj"], cpu["obj"], rtol=1e-9, atol=1e-9)
    assert np.isin(cpu["exitflag"], (1, 2)).all()   # (every plan was compared)


def _against_oracle(rt, name, B, seed, **kw):
    sc = rt["make_scenario"](name, B=B, seed=seed, **kw)
    cpu = rt["Oracle"](sc.desc).solve_batch(sc.xinit, sc.x0, sc.params)
    s = rt["Solver"](sc.desc, max_batch=B)
    fused = s.is_fused()
    gpu = s.solve(sc.xinit, sc.x0, sc.params)
    s.close()
    _compare(name, kw, B, gpu, cpu, sc.desc["nx"] + sc.desc["ns"])
    return fused


@pytest.mark.parametrize("N", [2, 3, 4, 29, 30, 31, 32])
def test_point_robot_horizons(rt, N):
    assert _against_oracle(rt, "cfg2", 3, 300 + N, time_horizon=N)


def test_one_half_enters_the_call(rt, monkeypatch):
    monkeypatch.delenv("RMPC_NO_SPEC", raising=False)
    assert _against_oracle(rt, "cfg1", 1, 1)


def test_chain2_other_broadcast_lanes(rt):
    assert _against_oracle(rt, "chain2", 4, 312)


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from robot_mpcs_amd._lib import Solver
from robot_mpcs_amd.scenarios import make_scenario
sc = make_scenario("cfg2", B=5, seed=311)
s = Solver(sc.desc, max_batch=5)
assert s.is_fused() and s.spec_name() == ""
r = s.solve(sc.xinit, sc.x0, sc.params)
s.close()
np.savez(sys.argv[2], **{k: r[k] for k in ("z", "exitflag", "iters", "kkt", "obj")})
"""


def test_runtime_tables_in_a_fresh_process(rt, tmp_path):
    sc = rt["make_scenario"]("cfg2", B=5, seed=311)
    cpu = rt["Oracle"](sc.desc).solve_batch(sc.xinit, sc.x0, sc.params)
    out = str(tmp_path / "nospec.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    subprocess.run([sys.executable] + flags + ["-c", _CHILD, ROOT, out], check=True, timeout=300,
                   env=dict(os.environ, RMPC_NO_SPEC="1"))
    gpu = dict(np.load(out))
    _compare("cfg2 (runtime tables)", {}, 5, gpu, cpu, sc.desc["nx"] + sc.desc["ns"])


def test_work_area_is_the_calls_own_and_idle_lanes_stay_out(rt):
    """poison_lds() fills the LDS of every CU, the scratch memory and the workspace with NaN patterns: a solve after it
    returns bit for bit what the solve before it returned, and that is the oracle's."""
    B = 5
    sc = rt["make_scenario"]("cfg2", B=B, seed=313, time_horizon=3)
    cpu = rt["Oracle"](sc.desc).solve_batch(sc.xinit, sc.x0, sc.params)
    s = rt["Solver"](sc.desc, max_batch=B)
    assert s.is_fused()
    clean = s.solve(sc.xinit, sc.x0, sc.params)
    s.poison_lds()
    dirty = s.solve(sc.xinit, sc.x0, sc.params)
    s.close()
    assert np.array_equal(clean["exitflag"], dirty["exitflag"]) and np.array_equal(clean["iters"], dirty["iters"])
    assert np.array_equal(clean["z"], dirty["z"])
    _compare("cfg2 after poison_lds", dict(time_horizon=3), B, dirty, cpu, sc.desc["nx"] + sc.desc["ns"])
    _compare("cfg2 before poison_lds", dict(time_horizon=3), B, clean, cpu, sc.desc["nx"] + sc.desc["ns"])


def _oracle_log(oracle, sc, b):
    """the oracle's iteration log (ORC_TRACE: standard error of the C library) of instance b"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tf:
        keep = os.dup(2)
        os.dup2(tf.fileno(), 2)
        try:
            oracle.solve(sc.xinit[b], sc.x0[b], sc.params[b])
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tf.seek(0)
        return tf.read().decode()


def _turned_down_curvature_steps(log):
    """Iterations of one oracle solve whose step was computed with the Gauss-Newton blocks although the barrier parameter
    was below the level (1e-2) from which the point robot's step takes the exact curvature: the curvature step was
    turned down first -- its factorisation failed or its line search rejected it -- and the iteration fell back.  (The
    latch that skips curvature steps only closes after such iterations, so the first of them is never the latch's.)"""
    mu, n = None, 0
    for ln in log.split("\n"):
        m = re.search(r"orc it\s+\d+ .* mu (\S+) obj", ln)
        if m:
            mu = float(m.group(1))
            continue
        m = re.search(r"step alpha .* curv (\d)", ln)
        if m and mu is not None and int(m.group(1)) == 0 and mu < 0.99e-2:   # (mu is printed to three digits)
            n += 1
    return n


def test_all_lanes_agree_on_the_factorisation_flag(rt, monkeypatch):
    """inst_after_recursion runs per lane on the flag ric_point_robot returns.  Seed 6 is the first cfg2 batch of eight
    (seeds 0 .. 299 tried with the oracle) in which an instance -- instance 3, twice in its 24 iterations -- has a
    curvature step turned down and falls back to the Gauss-Newton blocks; the oracle's log is read here again to hold
    that, and the batch is held to the oracle like every other."""
    B, seed = 8, 6
    sc = rt["make_scenario"]("cfg2", B=B, seed=seed)
    orc = rt["Oracle"](sc.desc)
    monkeypatch.setenv("ORC_TRACE", "1")
    counts = [_turned_down_curvature_steps(_oracle_log(orc, sc, b)) for b in range(B)]
    monkeypatch.delenv("ORC_TRACE")
    print("curvature steps turned down per instance (oracle):", counts)
    assert max(counts) >= 1
    assert _against_oracle(rt, "cfg2", B, seed)


def test_arm_sums_over_eight_lanes_unchanged(rt):
    assert _against_oracle(rt, "cfg4", 2, 314)
