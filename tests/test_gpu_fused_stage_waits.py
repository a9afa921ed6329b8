"""The stage loops that one wavefront runs alone in k_fused, with nothing pending at their loop headers: the backward
loop of the point robot's recursion (ric_point_robot) takes the record of its first stage from requests made in front of
the loop, and an explicit wait (lds_requests_done) completes them there, so that no stage waits at its top for the image
stores of the stage before it.  The sweep of the chain without slack finalises a variable right behind its rows under a
generated view.  No floating-point operation changes, so every case is held to the oracle at the bars of
tests/test_gpu_parity.py (check_plan: equal flags, iteration counts, plans to 1e-6 relative), and the oracle ends every
instance of every case with flag 1 or 2, so every plan is compared.  The wait stands where the loop's first stage takes
its record: the cases are the shapes that enter and leave the loops differently.

  cfg2, horizons 1, 2, 3, 30, 32, B = 3   one stage: the record requested in front of the loop is the only one, and the
                                          rollout is its first stage alone; 2, 3: the rollout's tail, one stage or two; 30,
                                          32: pairs with and without the tail, the first record at the far end of the 32
                                          slots; B = 3: one wavefront with both halves busy, one with an idle half
  cfg1, B = 1                             the smallest single instance (the other generated view)
  chain2, B = 4                           the other model of the path (n = 2: other strides, other idle lanes)
  cfg2, RMPC_NO_SPEC=1, fresh process     the runtime tables (the variable is read when a handle is created): the sweep
                                          that finalises all variables at the end, in front of the same recursion
  cfg2, N = 3, after poison_lds()         bit for bit the clean solve: a record taken before it had arrived would be a
                                          stale one, NaN patterns here

(No loop of the boxer's path was changed: its waits guard requests the stage itself made)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_support import check_plan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, B, seed, scenario keywords): seeds for which the oracle ends every instance with flag 1 or 2
HORIZON_SEED = {1: 301, 2: 302, 3: 303, 30: 330, 32: 332}
NOSPEC_SEED, CHAIN2_SEED, POISON_SEED = 341, 342, 343


@pytest.fixture(scope="module")
def rt():
    import __graft_entry__ as g
    g.build()
    from oracle.oracle import Oracle
    from robot_mpcs_amd._lib import Solver
    from robot_mpcs_amd.scenarios import make_scenario
    return dict(Oracle=Oracle, Solver=Solver, make_scenario=make_scenario)


def _oracle(rt, sc):
    cpu = rt["Oracle"](sc.desc).solve_batch(sc.xinit, sc.x0, sc.params)
    assert np.isin(cpu["exitflag"], (1, 2)).all(), cpu["exitflag"]   # (every plan is compared)
    return cpu


def _compare(what, gpu, cpu, sc):
    print("%s: flags %s, iterations gpu %s oracle %s, max plan error %.3e" % (
        what, gpu["exitflag"].tolist(), gpu["iters"].tolist(), cpu["iters"].tolist(), np.abs(gpu["z"] - cpu["z"]).max()))
    check_plan(gpu, cpu, sc.desc["nx"] + sc.desc["ns"])
    np.testing.assert_allclose(gpu["obj"], cpu["obj"], rtol=1e-9, atol=1e-9)


def _against_oracle(rt, name, B, seed, **kw):
    sc = rt["make_scenario"](name, B=B, seed=seed, **kw)
    cpu = _oracle(rt, sc)
    s = rt["Solver"](sc.desc, max_batch=B)
    fused = s.is_fused()
    gpu = s.solve(sc.xinit, sc.x0, sc.params)
    s.close()
    _compare("%s %s B=%d" % (name, kw, B), gpu, cpu, sc)
    return fused


@pytest.mark.parametrize("N", sorted(HORIZON_SEED))
def test_point_robot_first_record_at_every_way_into_the_loops(rt, N, monkeypatch):
    monkeypatch.delenv("RMPC_NO_SPEC", raising=False)
    assert _against_oracle(rt, "cfg2", 3, HORIZON_SEED[N], time_horizon=N)


def test_smallest_single_instance(rt, monkeypatch):
    monkeypatch.delenv("RMPC_NO_SPEC", raising=False)
    assert _against_oracle(rt, "cfg1", 1, 0)


def test_chain2_takes_the_same_path(rt):
    assert _against_oracle(rt, "chain2", 4, CHAIN2_SEED)


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from robot_mpcs_amd._lib import Solver
from robot_mpcs_amd.scenarios import make_scenario
sc = make_scenario("cfg2", B=5, seed=int(sys.argv[3]))
s = Solver(sc.desc, max_batch=5)
assert s.is_fused() and s.spec_name() == ""
r = s.solve(sc.xinit, sc.x0, sc.params)
s.close()
np.savez(sys.argv[2], **{k: r[k] for k in ("z", "exitflag", "iters", "kkt", "obj")})
"""


def test_runtime_tables_in_a_fresh_process(rt, tmp_path):
    sc = rt["make_scenario"]("cfg2", B=5, seed=NOSPEC_SEED)
    cpu = _oracle(rt, sc)
    out = str(tmp_path / "nospec.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    subprocess.run([sys.executable] + flags + ["-c", _CHILD, ROOT, out, str(NOSPEC_SEED)], check=True, timeout=300,
                   env=dict(os.environ, RMPC_NO_SPEC="1"))
    _compare("cfg2 over the runtime tables", dict(np.load(out)), cpu, sc)


def test_no_stale_record_after_poisoned_lds(rt, monkeypatch):
    """poison_lds() fills the LDS of every CU, the scratch memory and the workspace with NaN patterns: a solve after it
    returns bit for bit what the solve before it returned, and that is the oracle's.  With three stages the record
    requested in front of the backward loop is a third of all records."""
    monkeypatch.delenv("RMPC_NO_SPEC", raising=False)
    B = 3
    sc = rt["make_scenario"]("cfg2", B=B, seed=POISON_SEED, time_horizon=3)
    cpu = _oracle(rt, sc)
    s = rt["Solver"](sc.desc, max_batch=B)
    assert s.is_fused()
    clean = s.solve(sc.xinit, sc.x0, sc.params)
    s.poison_lds()
    dirty = s.solve(sc.xinit, sc.x0, sc.params)
    s.close()
    for key in ("exitflag", "iters", "z", "obj", "kkt"):
        assert np.array_equal(clean[key], dirty[key]), key
    _compare("cfg2 N=3 after poison_lds", dirty, cpu, sc)
