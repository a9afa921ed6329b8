"""The stage loops of the point robot's recursion in k_fused (ric_point_robot) without their bookkeeping: every LDS
access of a stage is base + k * stride with a per-lane base and stride set before the loop (a lane without the access
has stride 0 and a dummy word, a lane whose block position takes no diagonal or defect entry reads a zero of the work
area), the next stage's record is requested into the registers phase A has just emptied, the rollout runs two stages
per turn behind a first stage of its own, both loops count in scalar registers, and the DPP moves have no `old` operand.
No floating-point operation changes, so every case is held to the oracle at the bars of tests/test_gpu_parity.py
(equal flags, iteration counts, plans to 1e-6 relative), at the smallest shapes that take each path:

  horizons 2, 3, 4, 29, 30, 31, 32, B = 3   the rollout's first stage alone / with the odd stage behind the pairs / with
                                            pairs only, the backward loop's first and last request at both ends of the 32
                                            slots; B = 3: one wavefront with both halves busy, one with an idle half
  cfg1 (B = 1), cfg2 (B = 5)                both generated views
  cfg2, RMPC_NO_SPEC=1, fresh process       the runtime tables (the variable is read when a handle is created)
  chain2, B = 4                             the other model of the path (n = 2: other strides, other idle lanes)
  cfg2, N = 3, after poison_lds()           the zeros of the work area and the dummy words are the call's own
  cfg4, B = 2                               dpp_sum8 (the arms) is built from the same moves
"""
import os
import subprocess
import sys

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


def _against_oracle(rt, name, B, seed, **kw):
    sc = rt["make_scenario"](name, B=B, seed=seed, **kw)
    cpu = rt["Oracle"](sc.desc).solve_batch(sc.xinit, sc.x0, sc.params)
    s = rt["Solver"](sc.desc, max_batch=B)
    fused = s.is_fused()
    gpu = s.solve(sc.xinit, sc.x0, sc.params)
    s.close()
    print("%s %s B=%d: flags %s, iterations gpu %s oracle %s, max plan error %.3e" % (
        name, kw, B, gpu["exitflag"].tolist(), gpu["iters"].tolist(), cpu["iters"].tolist(), np.abs(gpu["z"] - cpu["z"]).max()))
    check_plan(gpu, cpu, sc.desc["nx"] + sc.desc["ns"])
    np.testing.assert_allclose(gpu["obj"], cpu["obj"], rtol=1e-9, atol=1e-9)
    assert np.isin(cpu["exitflag"], (1, 2)).all()   # (every plan was compared)
    return fused


@pytest.mark.parametrize("N", [2, 3, 4, 29, 30, 31, 32])
def test_point_robot_horizons_pairs_and_tail(rt, N):
    assert _against_oracle(rt, "cfg2", 3, 200 + N, time_horizon=N)


@pytest.mark.parametrize("name,B,seed", [("cfg1", 1, 0), ("cfg2", 5, 211)])
def test_generated_views(rt, name, B, seed, monkeypatch):
    monkeypatch.delenv("RMPC_NO_SPEC", raising=False)
    assert _against_oracle(rt, name, B, seed)


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from robot_mpcs_amd._lib import Solver
from robot_mpcs_amd.scenarios import make_scenario
sc = make_scenario("cfg2", B=5, seed=211)
s = Solver(sc.desc, max_batch=5)
assert s.is_fused() and s.spec_name() == ""
r = s.solve(sc.xinit, sc.x0, sc.params)
s.close()
np.savez(sys.argv[2], **{k: r[k] for k in ("z", "exitflag", "iters", "kkt", "obj")})
"""


def test_runtime_tables_in_a_fresh_process(rt, tmp_path):
    sc = rt["make_scenario"]("cfg2", B=5, seed=211)
    cpu = rt["Oracle"](sc.desc).solve_batch(sc.xinit, sc.x0, sc.params)
    out = str(tmp_path / "nospec.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    subprocess.run([sys.executable] + flags + ["-c", _CHILD, ROOT, out], check=True, timeout=300,
                   env=dict(os.environ, RMPC_NO_SPEC="1"))
    gpu = dict(np.load(out))
    print("runtime tables: flags %s, iterations gpu %s oracle %s, max plan error %.3e" % (
        gpu["exitflag"].tolist(), gpu["iters"].tolist(), cpu["iters"].tolist(), np.abs(gpu["z"] - cpu["z"]).max()))
    check_plan(gpu, cpu, sc.desc["nx"] + sc.desc["ns"])
    np.testing.assert_allclose(gpu["obj"], cpu["obj"], rtol=1e-9, atol=1e-9)


def test_chain2_takes_the_same_path(rt):
    assert _against_oracle(rt, "chain2", 4, 212)


def test_zeros_and_dummy_words_are_the_calls_own(rt):
    """poison_lds() fills the LDS of every CU, the scratch memory and the workspace with NaN patterns: a solve after it
    returns bit for bit what the solve before it returned (tests/test_gpu_parity.py, stale LDS), and that is the oracle's."""
    B = 5
    sc = rt["make_scenario"]("cfg2", B=B, seed=213, time_horizon=3)
    cpu = rt["Oracle"](sc.desc).solve_batch(sc.xinit, sc.x0, sc.params)
    s = rt["Solver"](sc.desc, max_batch=B)
    assert s.is_fused()
    clean = s.solve(sc.xinit, sc.x0, sc.params)
    s.poison_lds()
    dirty = s.solve(sc.xinit, sc.x0, sc.params)
    s.close()
    assert np.array_equal(clean["exitflag"], dirty["exitflag"]) and np.array_equal(clean["iters"], dirty["iters"])
    assert np.array_equal(clean["z"], dirty["z"])
    check_plan(dirty, cpu, sc.desc["nx"] + sc.desc["ns"])


def test_arm_sums_over_eight_lanes_unchanged(rt):
    assert _against_oracle(rt, "cfg4", 2, 214)
