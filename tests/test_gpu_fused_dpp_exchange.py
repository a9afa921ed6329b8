"""The fused kernels with the lane exchanges of their pass path as vector moves: the whole-horizon reductions of the sweep
call (wave_reduce_many: permlane swaps and DPP row moves instead of the LDS crossbar) and the rollout of the point
robot's recursion (ric_point_robot: dx handed round in registers by DPP row moves instead of a store, an ordering point
and a read-back per stage).  Both are arithmetic-neutral, so the bar is the one of tests/test_gpu_parity.py -- flags,
iteration counts and plans against the CPU oracle (check_plan), the objective to 1e-9, every oracle flag 1 or 2 -- at
the smallest shapes that take each path: the rollout's first stage alone (N = 2), an odd stage behind the pairs of its
loop (N = 3, 29, 31) and none (N = 4, 30, 32), both ends of the 32 slots, an idle half (odd B; B = 1), the gantry's lanes
(chain2), the reductions in the body of k_fused (cfg3), the 64-lane tree (the pass kernels of chain4; cfg4's k_fused_arm,
whose sweep call keeps the shuffle form, is held to the same bar), half-wavefront instances of the pass kernels with a
half that returns early (cfg2 through k_riccati's grouped blocks), the runtime tables instead of the generated view
(RMPC_NO_SPEC=1), and a solve after rmpc_debug_poison_lds.

Seeds: the first seed from 301 on (one per case, in the order below) whose oracle run ends every instance with flag 1
or 2; none had to be skipped."""
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


def _against_oracle(rt, sc, gpu):
    cpu = rt["Oracle"](sc.desc).solve_batch(sc.xinit, sc.x0, sc.params)
    assert np.all(np.isin(cpu["exitflag"], (1, 2))), cpu["exitflag"]
    check_plan(gpu, cpu, sc.desc["nx"] + sc.desc["ns"])
    np.testing.assert_allclose(gpu["obj"], cpu["obj"], rtol=1e-9, atol=1e-9)


CASES = [
    # (name, B, seed, scenario overrides, environment, fused kernel expected)
    ("cfg2", 3, 301, {"time_horizon": 2}, {}, True), ("cfg2", 3, 302, {"time_horizon": 3}, {}, True),
    ("cfg2", 3, 303, {"time_horizon": 4}, {}, True), ("cfg2", 3, 304, {"time_horizon": 29}, {}, True),
    ("cfg2", 3, 305, {"time_horizon": 30}, {}, True), ("cfg2", 3, 306, {"time_horizon": 31}, {}, True),
    ("cfg2", 3, 307, {"time_horizon": 32}, {}, True),
    ("cfg1", 1, 308, {}, {}, True),
    ("chain2", 4, 309, {}, {}, True),
    ("cfg3", 3, 310, {}, {}, True),
    ("cfg4", 2, 311, {}, {}, True),
    # the pass kernels: a wavefront per instance (chain4), and half a wavefront per instance in k_riccati's grouped
    # blocks (lists of 512 instances and more; 513: the last block holds one instance, its partner half returns early)
    ("chain4", 3, 312, {}, {}, False),
    ("cfg2", 513, 313, {}, {"RMPC_NO_FUSED": "1"}, False),
]


@pytest.mark.parametrize("name,B,seed,kw,env,fused", CASES)
def test_paths_match_oracle(rt, name, B, seed, kw, env, fused, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)   # (read at rmpc_create)
    sc = rt["make_scenario"](name, B=B, seed=seed, **kw)
    s = rt["Solver"](sc.desc, max_batch=B)
    assert s.is_fused() == fused
    gpu = s.solve(sc.xinit, sc.x0, sc.params)
    s.close()
    _against_oracle(rt, sc, gpu)


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from robot_mpcs_amd._lib import Solver
from robot_mpcs_amd.scenarios import make_scenario
sc = make_scenario("cfg2", B=5, seed=314)
s = Solver(sc.desc, max_batch=5)
assert s.is_fused() and s.spec_name() == "", s.spec_name()
r = s.solve(sc.xinit, sc.x0, sc.params)
s.close()
np.savez(sys.argv[2], **r)
"""


def test_runtime_tables_match_oracle(rt, tmp_path):
    """RMPC_NO_SPEC=1 (the fused kernel over the runtime tables: the sweep and the step lengths are calls of their own
    and the reductions run in the kernel's body), in a fresh process: the variable is part of that process from its
    start."""
    out = str(tmp_path / "nospec.npz")
    env = dict(os.environ, RMPC_NO_SPEC="1")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], check=True, env=env, timeout=120)
    gpu = dict(np.load(out))
    sc = rt["make_scenario"]("cfg2", B=5, seed=314)
    _against_oracle(rt, sc, gpu)


def test_rollout_does_not_depend_on_stale_lds(rt):
    """cfg2, B = 5, N = 3: the rollout keeps dx in registers and its image rows a stage ahead; nothing it reads may be
    left over from an earlier kernel -- a solve after rmpc_debug_poison_lds equals the solve before it bit for bit."""
    sc = rt["make_scenario"]("cfg2", B=5, seed=315, time_horizon=3)
    s = rt["Solver"](sc.desc, max_batch=5)
    clean = s.solve(sc.xinit, sc.x0, sc.params)
    s.poison_lds()
    dirty = s.solve(sc.xinit, sc.x0, sc.params)
    s.close()
    for key in ("z", "exitflag", "iters", "obj", "kkt"):
        assert np.array_equal(clean[key], dirty[key]), key
    _against_oracle(rt, sc, clean)
