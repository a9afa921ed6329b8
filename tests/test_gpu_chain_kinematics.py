"""The kernels' kinematics and curvature on chains that mix revolute and prismatic joints (chain_cases.py; DESIGN.md
6.3): what test_chain_kinematics_cpu.py pins on the oracle, here on every path of the library a class can run.  The
shipped chains never take the prismatic branches of the arms' slot code (rmpc_arm_fused.hpp) and of Kin<C> with more
than three joints (rmpc_model.hpp), the joint-type guard of k_sweep's FKCURV block (rmpc_sweep.hpp), Rodrigues'
formula off local z, an origin rotation with pitch or yaw, or Cfg::CURV compiled in with the terms off at run time.

  class                      paths
  mix2, mix3, aff3, aff3g    k_fused over the runtime tables; RMPC_NO_FUSED=1 (pass kernels); RMPC_NO_FUSED=1
                             RMPC_RIC_LANE=2 (mix3 and aff3g)
  mix5, mix7                 k_fused_arm three parts; RMPC_ARM_TWO_PARTS=1; RMPC_NO_FUSED=1 (k_sweep's FKCURV branch,
                             ric_arm_block in k_riccati)
  mix4, mix8                 pass kernels, ric_backward
Every case asserts the path it ran: is_fused, the path words of rmpc_debug_step, last_solve_path.

Checks: the sweep's blocks against numpy with the returned t, lam and mu and the Newton step against the refined dense
KKT solve (test_gpu_newton_step.py's, B = 6, cold and late, at the class's own N of 10 to 12: over four stages no
converged plan of these chains has a row at the warm-start clamp, which the late inputs need; mix4 and mix5 also at
B = 520 through the grouped pass kernels); the curvature terms and the step on the exact Hessian
(exact_hessian_cases.py (a), (b), (c), B = 4, N = 4, cold and conv; C == 0 and a step that does not depend on the weight
for the classes without terms); whole solves at the class's own N, B = 32: a cold solve and three warm control steps
against the oracle under check_plan.

Measured on an MI355X (table per path: DESIGN.md 6.3): step error over the textbook recursion's at most 2.96 (aff3,
pass kernels, late; bound 16), on the exact Hessian at most 3.22 (mix7, k_fused_arm, conv); |C - C_ref| / scale at most
1.22e-11 (mix5 conv, the same on its three paths; bound u + 9.0e-10), the oracle's figures; every whole solve and warm
step with the oracle's iteration counts.
"""
import functools

import numpy as np
import pytest

import chain_cases as cc
import exact_hessian_cases as ehc
import kkt_reference as ref
import newton_step_cases as nsc
from gpu_support import check_plan
from test_gpu_newton_step import _check_blocks

pytestmark = pytest.mark.gpu

NOF = {"RMPC_NO_FUSED": "1"}
LANE = {"RMPC_NO_FUSED": "1", "RMPC_RIC_LANE": "2"}
TWO = {"RMPC_ARM_TWO_PARTS": "1"}
H4 = {"time_horizon": 4}

# path -> (environment at rmpc_create, fused handle?, path words of rmpc_debug_step, recursion kernel of a whole solve)
PATHS = {
    "fused": ({}, True, dict(fused="k_fused", generated_view=False), None),
    "arm3": ({}, True, dict(fused="k_fused_arm", arm_parts=3, generated_view=False), None),
    "arm2": (TWO, True, dict(fused="k_fused_arm", arm_parts=2, generated_view=False), None),
    "pass": ({}, False, dict(fused="", ric_lane=1, generated_view=False), "wave"),
    "nofused": (NOF, False, dict(fused="", ric_lane=1, generated_view=False), "wave"),
    "lane": (LANE, False, dict(fused="", ric_lane=2, generated_view=False), "lane"),
}
FAMILY_PATHS = {"small": ("fused", "nofused"), "arm": ("arm3", "arm2", "nofused"), "pass": ("pass",)}
# (class, path)
CASES = ([(n, p) for n in cc.NAMES for p in FAMILY_PATHS[cc.CLASSES[n]["family"]]]
         + [("mix3", "lane"), ("aff3g", "lane")])
# the exact-Hessian hook: the arms on their three paths, the pass-kernel chains, the small chains on k_fused (the
# lane-per-instance kernel takes its weight from the instance: test_gpu_exact_hessian.py)
HESSIAN_CASES = [(n, p) for n, p in CASES if p not in ("lane",) and (cc.CLASSES[n]["family"] != "small" or p == "fused")]
GROUPED = [("mix4", "pass"), ("mix5", "nofused")]
GROUPED_B = 520   # >= kGroupedMin, no multiple of 64 or of the six distinct instances


def _id(c):
    return "%s-%s" % c


def _open(rt, monkeypatch, sc, path, B):
    env, fused, _, _ = PATHS[path]
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)   # (read once, at rmpc_create)
    assert rt["spec_for"](sc.desc) == ""   # (no generated view of these models: the runtime tables)
    s = rt["Solver"](sc.desc, max_batch=B)
    assert s.is_fused() == fused, path
    return s


def _check_path(d, path):
    for key, want in PATHS[path][2].items():
        assert d["path"][key] == want, (key, d["path"])


@pytest.fixture(scope="module")
def rt():
    import __graft_entry__ as g
    g.build()
    from oracle.oracle import Oracle
    from robot_mpcs_amd._lib import Solver, spec_for
    step_inputs = functools.lru_cache(maxsize=None)(
        lambda name, mode: nsc.make_inputs(cc.make_chain_scenario, Oracle, name, mode, 6))

    @functools.lru_cache(maxsize=None)
    def prepared(name, mode):
        sc, o, xinit, x0, params, duals = ehc.make_inputs(cc.make_chain_scenario, Oracle, name, mode, H4)
        refs = [ehc.instance_reference(o, mode, xinit, x0, params, duals, b) for b in range(ehc.B)]
        return sc, o, xinit, x0, params, duals, refs

    @functools.lru_cache(maxsize=None)
    def closed_loop(name):
        """The class at its own N, B = 32: the oracle's cold solve and three warm control steps (plant: the model's map,
        start of a step: the shifted plan of the oracle), with the inputs of every step."""
        B = 32
        sc = cc.make_chain_scenario(name, B=B, seed=nsc.case_seed(name, "loop"))
        o = Oracle(sc.desc)
        nxs = o.nx + o.ns
        x, x0, duals, steps = sc.xinit.copy(), sc.x0.copy(), [None] * B, []
        for t in range(4):
            rs = [o.solve_warm(x[b], x0[b], sc.params[b], duals[b]) for b in range(B)]
            cpu = dict(z=np.array([r["z"] for r in rs]), exitflag=np.array([r["exitflag"] for r in rs], dtype=np.int32),
                       iters=np.array([r["iters"] for r in rs], dtype=np.int32), obj=np.array([r["obj"] for r in rs]))
            steps.append((x.copy(), x0.copy(), cpu))
            assert np.all(cpu["exitflag"] >= 1), (name, t, cpu["exitflag"])   # (the inputs: every plan converges)
            duals = [r["duals"] for r in rs]
            x = np.array([o.dynamics(x[b], cpu["z"][b, 0, nxs:]) for b in range(B)])
            x0 = np.concatenate([cpu["z"][:, 1:], cpu["z"][:, -1:]], axis=1)
        return sc, o, steps

    return dict(Solver=Solver, spec_for=spec_for, step_inputs=step_inputs, prepared=prepared, closed_loop=closed_loop)


def _step_case(rt, monkeypatch, name, path, mode, B):
    sc, o, xinit, x0, params, duals = rt["step_inputs"](name, mode)
    nd = xinit.shape[0]
    pick = np.arange(B) % nd
    s = _open(rt, monkeypatch, sc, path, B)
    d = s.debug_step(xinit[pick], x0[pick], params[pick], None if duals is None else tuple(a[pick] for a in duals))
    s.close()
    assert d["t"].shape[2] == o.m
    _check_path(d, path)
    assert np.all(d["ok"])
    for key in ("Q", "q0", "q1", "rc", "t", "lam", "mu", "dz", "nu"):   # copies of an instance: equal bit for bit
        assert np.array_equal(d[key], d[key][pick]), key
    errs, yard = [], []
    for b in range(nd):
        evals, z = nsc.stage_evals(o, xinit[b], x0[b], params[b])
        for k, e in enumerate(evals):
            e["z"] = z[k]
        _check_blocks(o, mode, d, b, evals, None if duals is None else duals[0][b], sc.desc["options"]["mu0"])
        A, Bm = nsc.dynamics_blocks(evals)
        q = d["q0"][b] - d["mu"][b] * d["q1"][b]
        dz_ref, nu_ref, e_text, rel = nsc.reference_and_yardstick(d["Q"][b], q, A, Bm, d["rc"][b])
        assert rel < ref.REFINE_TOL
        assert not np.any(d["nu"][b, 0])
        errs.append(ref.block_errors(d["dz"][b], d["nu"][b], dz_ref, nu_ref, o.nx, nu_from=1))
        yard.append(e_text)
        if mode == "cold":
            nsc.check_descent(ref.merit_slope(evals, z, d["t"][b], d["mu"][b], d["dz"][b], dz_ref), d["dz"][b])
    nsc.check_class("chain %s-%s B%d %s" % (name, path, B, mode), errs, yard)


@pytest.mark.parametrize("mode", nsc.MODES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_sweep_blocks_and_step_on_the_chains(rt, case, mode, monkeypatch):
    _step_case(rt, monkeypatch, case[0], case[1], mode, 6)


@pytest.mark.parametrize("mode", nsc.MODES)
@pytest.mark.parametrize("case", GROUPED, ids=_id)
def test_grouped_pass_kernels_on_the_chains(rt, case, mode, monkeypatch):
    _step_case(rt, monkeypatch, case[0], case[1], mode, GROUPED_B)


@pytest.mark.parametrize("mode", ehc.MODES)
@pytest.mark.parametrize("case", HESSIAN_CASES, ids=_id)
def test_exact_hessian_step_on_the_chains(rt, case, mode, monkeypatch):
    name, path = case
    sc, o, xinit, x0, params, duals, refs = rt["prepared"](name, mode)
    label = "chain %s-%s %s" % (name, path, mode)
    N, B = o.N, ehc.B
    noterms = not cc.CLASSES[name]["use_curv"]
    s = _open(rt, monkeypatch, sc, path, B)
    d = s.debug_step(xinit, x0, params, duals, curv=1.0)
    d0 = s.debug_step(xinit, x0, params, duals, curv=0.0)
    plain = s.debug_step(xinit, x0, params, duals)
    s.close()
    _check_path(d, path)
    for key in ("Q", "C", "q0", "q1", "rc", "t", "lam", "mu"):
        assert np.array_equal(d[key], d0[key]), key
    for key in ("Q", "q0", "q1", "rc", "t", "lam", "mu", "dz", "nu", "ok"):
        assert np.array_equal(d0[key], plain[key]), key
    assert np.all(plain["ok"])
    assert np.array_equal(d["C"], np.transpose(d["C"], (0, 1, 3, 2)))
    if noterms:   # Cfg::CURV compiled in, the terms off at run time
        assert not np.any(d["C"])
        for key in ("dz", "nu", "ok"):
            assert np.array_equal(d[key], d0[key]), key
    else:
        assert np.any(d["C"])
    insts, worst = [], 0.0
    for b, r in enumerate(refs):
        g = r["orc"]
        np.testing.assert_allclose(d["t"][b], g["t"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(d["lam"][b], g["lam"], rtol=1e-11, atol=0)
        assert d["mu"][b] == g["mu"]
        for k in range(N):
            np.testing.assert_allclose(d["Q"][b, k], g["Q"][k], rtol=1e-11, atol=1e-11 * max(1.0, np.abs(g["Q"][k]).max()))
        ehc.check_against_oracle("%s inst %d" % (label, b), d["C"][b], g["C"])                          # (a)
        if not noterms:
            worst = max(worst, ehc.check_against_reference("%s inst %d" % (label, b), d["C"][b], r))    # (b)
        A, Bm = nsc.dynamics_blocks(r["evals"])
        assert not np.any(d["nu"][b, 0])
        insts.append(dict(Q=d["Q"][b], C=d["C"][b], q=d["q0"][b] - d["mu"][b] * d["q1"][b], A=A, B=Bm, rc=d["rc"][b],
                          t=d["t"][b], mu=d["mu"][b], dz=d["dz"][b], nu=d["nu"][b], ok=d["ok"][b], evals=r["evals"], z=r["z"]))
    print("exact-hessian %s: |C - C_ref| / scale %.3e" % (label, worst))
    ehc.check_steps(label, mode, o, 1.0, insts, nu_from=1)                                              # (c)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_whole_solves_on_the_chains(rt, case, monkeypatch):
    """A cold solve, then a warm loop of three control steps, each against the oracle's solve of the same inputs."""
    name, path = case
    sc, o, steps = rt["closed_loop"](name)
    B, nxs = sc.B, o.nx + o.ns
    s = _open(rt, monkeypatch, sc, path, B)
    s.set_warm_start(True)
    for t, (x, x0, cpu) in enumerate(steps):
        gpu = s.solve(x, x0, sc.params)
        lp = s.last_solve_path()
        assert lp["fused"] == PATHS[path][1] and lp["ric_first"] == PATHS[path][3], (t, lp)
        print("chain %s-%s step %d: iterations gpu %.2f oracle %.2f" % (name, path, t, gpu["iters"].mean(), cpu["iters"].mean()))
        check_plan(gpu, cpu, nxs)
        if t == 0:
            np.testing.assert_allclose(gpu["obj"], cpu["obj"], rtol=1e-9, atol=1e-9)
    s.close()
