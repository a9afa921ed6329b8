"""The curvature terms and the curvature-weighted Newton step of every Riccati path of the library
(Solver.debug_step(curv=cw) = rmpc_debug_step_curv: one first sweep with the model's curvature terms, one recursion on
H = Q - cw C on the path the handle runs in production).  C is what the sweeps write to R_C / R_D of the stage records
-- Cqq of the distance rows and the inverse-barrier objective, the arms' blocks with the second derivatives of the
kinematics (k_sweep's FKCURV branch and the slot code of the fused arm sweep), the unicycle's frame rotation and
nu . grad^2 Phi -- placed into a dense matrix by the host.  Whole-solve parity cannot see an error in them: a converged
plan does not depend on the Hessian that was used.

Per case (exact_hessian_cases.py: inputs, bounds, figures): (a) C against the oracle's, (b) C against the difference
reference of hessian_reference.py, (c) the step and the recursion's return value against kkt_reference on the blocks the
hook returned -- ok == 0 for the instances whose reduced Hessian is not positive definite, which ordinary cold inputs
contain.  Also: the weight changes nothing but the step; the plain hook equals the new one at weight 0 bit for bit.

Paths and how a handle reaches them:
  fused point robot            cfg2, chain2 at their own N and N = 1, 2, 32; cw = 1/2 (Cfg::CSCALE); RMPC_NO_SPEC=1
  fused diff-drive             cfg3, boxer, wc_boxer_slack (slack column beside R_D); boxer at N = 2
  k_fused_arm, 3 and 2 parts   cfg4, chain5, chain6; RMPC_ARM_TWO_PARTS=1
  pass kernels                 cfg2, boxer, cfg4, chain4, chain8, wc_panda with RMPC_NO_FUSED=1
  k_riccati_lane               cfg2 with RMPC_NO_FUSED=1 RMPC_RIC_LANE=2.  That kernel takes its weight from the instance
                               (mu <= 1e-2: the instance's scale), so its cold case runs with the option mu0 = 1e-2 -- the
                               cold first pass of a solver configured to start there; the conv case is cfg2's own
  no terms                     cfg2 with the slack: C = 0, the step at cw = 1 is the step at cw = 0 bit for bit
N = 2: stage N - 1 carries no dynamics term.

Measured on an MI355X: |C - C_ref| / scale at most 1.12e-10 (point-cfg2-t32 conv; bound u + 9.0e-10), the same figures
as the oracle's; step error over the textbook recursion's at most 3.47 (pass-cfg2, lane-cfg2 conv; bound 16); 20 of the
116 cold instances are not positive definite and every path returns ok = 0 for them.
"""
import functools

import numpy as np
import pytest

import exact_hessian_cases as ehc
import newton_step_cases as nsc

pytestmark = pytest.mark.gpu

NOF = {"RMPC_NO_FUSED": "1"}
LANE = {"RMPC_NO_FUSED": "1", "RMPC_RIC_LANE": "2"}
TWO = {"RMPC_ARM_TWO_PARTS": "1"}
H = ehc.H
ARMS = ("cfg4", "chain5", "chain6")

PATHS = {
    "point": dict(fused="k_fused"), "half": dict(fused="k_fused"), "dd": dict(fused="k_fused"), "noterms": dict(fused="k_fused"),
    "nospec": dict(fused="k_fused", generated_view=False),
    "arm3": dict(fused="k_fused_arm", arm_parts=3), "arm2": dict(fused="k_fused_arm", arm_parts=2),
    "pass": dict(fused="", ric_lane=1), "lane": dict(fused="", ric_lane=2),
}

# (path, config, scenario overrides, environment, fused handle?, curvature weight)
CASES = (
    [("point", n, kw, {}, True, 1.0) for n in ("cfg2", "chain2") for kw in ({}, H(1), H(2), H(32))]
    + [("nospec", "cfg2", {}, {"RMPC_NO_SPEC": "1"}, True, 1.0)]
    + [("half", n, {}, {}, True, 0.5) for n in ("cfg2", "chain2")]
    + [("dd", n, {}, {}, True, 1.0) for n in ("cfg3", "boxer", "wc_boxer_slack")] + [("dd", "boxer", H(2), {}, True, 1.0)]
    + [("arm3", n, {}, {}, True, 1.0) for n in ARMS] + [("arm2", n, {}, TWO, True, 1.0) for n in ARMS]
    + [("pass", n, {}, NOF, False, 1.0) for n in ("cfg2", "boxer", "cfg4", "chain4", "chain8", "wc_panda")]
    + [("lane", "cfg2", {}, LANE, False, 1.0)]
    + [("noterms", "cfg2", {"slack": True}, {}, True, 1.0)]
)
LANE_COLD = {"mu0": 1e-2}


def _id(c):
    return "%s-%s" % (c[0], ehc.class_id(c[1], c[2]))


@pytest.fixture(scope="module")
def rt():
    import __graft_entry__ as g
    g.build()
    from oracle.oracle import Oracle
    from robot_mpcs_amd._lib import Solver, spec_for
    from robot_mpcs_amd.scenarios import make_scenario

    @functools.lru_cache(maxsize=None)
    def prepared(name, mode, kw):
        sc, o, xinit, x0, params, duals = ehc.make_inputs(make_scenario, Oracle, name, mode, kw)
        refs = [ehc.instance_reference(o, mode, xinit, x0, params, duals, b) for b in range(ehc.B)]
        return sc, o, xinit, x0, params, duals, refs

    return dict(Solver=Solver, prepared=prepared, spec_for=spec_for)


@pytest.mark.parametrize("mode", ehc.MODES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_exact_hessian_step(rt, case, mode, monkeypatch):
    path, name, kw, env, fused, cw = case
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)   # (read once, at rmpc_create)
    if path == "lane" and mode == "cold":
        kw = dict(kw, **LANE_COLD)
    sc, o, xinit, x0, params, duals, refs = rt["prepared"](name, mode, tuple(sorted(kw.items())))
    label = "%s %s" % (_id(case), mode)
    N, nx, B = o.N, o.nx, ehc.B
    s = rt["Solver"](sc.desc, max_batch=B)
    assert s.is_fused() == fused
    d = s.debug_step(xinit, x0, params, duals, curv=cw)
    d0 = s.debug_step(xinit, x0, params, duals, curv=0.0)
    plain = s.debug_step(xinit, x0, params, duals)
    s.close()
    for key, want in PATHS[path].items():
        assert d["path"][key] == want, (key, d["path"])
    view = rt["spec_for"](sc.desc)
    assert path != "nospec" or view != ""
    assert d["path"]["generated_view"] == (view != "" and path != "nospec")
    # the weight changes the step and nothing else; the plain hook is the new one at weight 0 without C
    for key in ("Q", "C", "q0", "q1", "rc", "t", "lam", "mu"):
        assert np.array_equal(d[key], d0[key]), key
    for key in ("Q", "q0", "q1", "rc", "t", "lam", "mu", "dz", "nu", "ok"):
        assert np.array_equal(d0[key], plain[key]), key
    assert np.all(plain["ok"])
    assert np.array_equal(d["C"], np.transpose(d["C"], (0, 1, 3, 2)))
    if path == "noterms":
        assert not np.any(d["C"])
        for key in ("dz", "nu", "ok"):
            assert np.array_equal(d[key], d0[key]), key
    if N == 2:   # stage N - 1 carries no dynamics term: nothing outside the q block
        assert not np.any(d["C"][:, N - 1, o.n:, :]) and not np.any(d["C"][:, N - 1, :, o.n:])
    insts, worst = [], 0.0
    for b, r in enumerate(refs):
        g = r["orc"]
        # the reference was formed with the oracle's multipliers: the path's are the same numbers
        np.testing.assert_allclose(d["t"][b], g["t"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(d["lam"][b], g["lam"], rtol=1e-11, atol=0)
        assert d["mu"][b] == g["mu"]
        for k in range(N):
            np.testing.assert_allclose(d["Q"][b, k], g["Q"][k], rtol=1e-11, atol=1e-11 * max(1.0, np.abs(g["Q"][k]).max()))
        ehc.check_against_oracle("%s inst %d" % (label, b), d["C"][b], g["C"])                            # (a)
        if path != "noterms":
            worst = max(worst, ehc.check_against_reference("%s inst %d" % (label, b), d["C"][b], r))    # (b)
        A, Bm = nsc.dynamics_blocks(r["evals"])
        assert not np.any(d["nu"][b, 0])
        insts.append(dict(Q=d["Q"][b], C=d["C"][b], q=d["q0"][b] - d["mu"][b] * d["q1"][b], A=A, B=Bm, rc=d["rc"][b],
                          t=d["t"][b], mu=d["mu"][b], dz=d["dz"][b], nu=d["nu"][b], ok=d["ok"][b], evals=r["evals"], z=r["z"]))
    print("exact-hessian %s: |C - C_ref| / scale %.3e" % (label, worst))
    ehc.check_steps(label, mode, o, cw, insts, nu_from=1)                                                # (c)
