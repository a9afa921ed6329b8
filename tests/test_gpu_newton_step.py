"""The Newton step of every Riccati path of the library (Solver.debug_step: one first sweep and one recursion on the
path the handle runs in production) against the refined dense KKT solution of the condensed QP built from the blocks
the hook returned -- step dz, new costates nu+ and the recursion's return value.  A converged plan cannot tell a
slightly wrong step from a right one (the iteration corrects itself); this can.  Bound, modes and inputs:
newton_step_cases.py; reference: kkt_reference.py.  A and B come from Oracle.eval_stage.  nu+ is compared from stage 1
on: the costate of stage 0 multiplies the fixed first state, no kernel path forms it (the rollouts store nu+ for
k >= 1), no residual reads it, and the hook returns zeros there (the oracle forms it; test_newton_step_cpu.py compares it).

In the same test the returned blocks are checked against the numpy formula of test_sweep_blocks_match_oracle evaluated
with the returned t, lam and mu, at that test's tolerances, and t / lam against the cold and the warm start rule: the
warm first pass at block level.

Paths (riccati_recursion in rmpc_riccati.hpp picks one; each is in the header named in brackets) and how a handle
reaches them:
  ric_point_robot           fused, chains n <= 3 without slack        cfg2, chain2; N = 1, 2, 5, 31, 32      [rmpc_ric_point.hpp]
  ric_chain_slack_backward  fused, point robot with the slack        cfg2 slack; the same horizons           [rmpc_ric_slack.hpp]
  ric_dd_backward           fused, diff-drive                         cfg3, boxer, wc_boxer_slack             [rmpc_ric_dd.hpp]
  ric_arm_block             k_fused_arm, three parts (3 N <= 64)     cfg4, chain5, chain6; N = 12, 17, 21    [rmpc_ric_arm.hpp]
  ric_arm_block             k_fused_arm, two parts                   the same, RMPC_ARM_TWO_PARTS=1; N = 22, 30 (no room for three)
  ric_arm_block             k_riccati (RMPC_NO_FUSED=1)               the same arms; N = 40 without the switch
  ric_backward              pass kernels                              chain4, chain8, wc_panda, boxer, cfg2 N = 40 [rmpc_ric_dense.hpp]
  k_riccati_lane            RMPC_NO_FUSED=1 RMPC_RIC_LANE=2           cfg2, chain2                            [rmpc_pass_riccati.hpp]
  runtime tables            RMPC_NO_SPEC=1                            cfg2
and one case per pass-kernel family at B = 520 >= kGroupedMin (eight instances tiled 65 times, not a multiple of 64):
copies equal bit for bit, each compared with its reference.
"""
import functools

import numpy as np
import pytest

import kkt_reference as ref
import newton_step_cases as nsc

pytestmark = pytest.mark.gpu

NOF = {"RMPC_NO_FUSED": "1"}
LANE = {"RMPC_NO_FUSED": "1", "RMPC_RIC_LANE": "2"}
TWO = {"RMPC_ARM_TWO_PARTS": "1"}
H = lambda N: {"time_horizon": N}
ARM_N = (12, 17, 21, 22, 30)
SMALL_N = (1, 2, 5, 31, 32)

# what Solver.debug_step reports of the handle's path, by the first entry of a case
PATHS = {
    "point": dict(fused="k_fused"), "slack": dict(fused="k_fused"), "dd": dict(fused="k_fused"),
    "nospec": dict(fused="k_fused", generated_view=False),
    "arm3": dict(fused="k_fused_arm", arm_parts=3), "arm2": dict(fused="k_fused_arm", arm_parts=2),
    "armpass": dict(fused="", ric_lane=1), "pass": dict(fused="", ric_lane=1), "grouped": dict(fused="", ric_lane=1),
    "lane": dict(fused="", ric_lane=2), "grouped-lane": dict(fused="", ric_lane=2),
}

# (path, config, scenario overrides, environment, fused handle?, copies of the distinct instances)
CASES = (
    [("point", n, kw, {}, True, 1) for n in ("cfg2", "chain2") for kw in [{}] + [H(N) for N in SMALL_N]]
    + [("slack", "cfg2", dict(slack=True, **kw), {}, True, 1) for kw in [{}] + [H(N) for N in SMALL_N]]
    + [("dd", n, {}, {}, True, 1) for n in ("cfg3", "boxer", "wc_boxer_slack")]
    + [("arm3", n, {}, {}, True, 1) for n in ("cfg4", "chain5", "chain6")] + [("arm3", "cfg4", H(N), {}, True, 1) for N in ARM_N if 3 * N <= 64]
    + [("arm2", n, {}, TWO, True, 1) for n in ("cfg4", "chain5", "chain6")] + [("arm2", "cfg4", H(N), TWO, True, 1) for N in ARM_N]
    + [("armpass", n, {}, NOF, False, 1) for n in ("cfg4", "chain5", "chain6")] + [("armpass", "cfg4", H(N), NOF, False, 1) for N in ARM_N]
    + [("armpass", "cfg4", H(40), {}, False, 1)]
    + [("pass", n, {}, NOF, False, 1) for n in ("chain4", "chain8", "wc_panda", "boxer")] + [("pass", "cfg2", H(40), {}, False, 1)]
    + [("lane", n, {}, LANE, False, 1) for n in ("cfg2", "chain2")]
    + [("nospec", "cfg2", {}, {"RMPC_NO_SPEC": "1"}, True, 1)]
    + [("grouped", "cfg2", {}, NOF, False, 65), ("grouped", "boxer", {}, NOF, False, 65), ("grouped", "cfg4", {}, NOF, False, 65),
       ("grouped-lane", "cfg2", {}, LANE, False, 65)]
)
DISTINCT = {1: 6, 65: 8}   # distinct instances of a case, by its number of copies


def _id(c):
    return "%s-%s" % (c[0], c[1]) + "".join("-%s%s" % (k[0], v) for k, v in sorted(c[2].items()))


@pytest.fixture(scope="module")
def rt():
    import __graft_entry__ as g
    g.build()
    from oracle.oracle import Oracle
    from robot_mpcs_amd._lib import Solver
    from robot_mpcs_amd.scenarios import make_scenario
    inputs = functools.lru_cache(maxsize=None)(
        lambda name, mode, B, kw: nsc.make_inputs(make_scenario, Oracle, name, mode, B, **dict(kw)))
    from robot_mpcs_amd._lib import spec_for
    return dict(Solver=Solver, inputs=inputs, spec_for=spec_for)


def _check_blocks(o, mode, d, b, evals, lam_w, mu0):
    """Blocks, slacks and multipliers of instance b against numpy, with the returned t, lam and mu."""
    N, nx = o.N, o.nx
    mu = d["mu"][b]
    assert mu == (mu0 if mode == "cold" else nsc.WARM_MU_MIN)
    for k, e in enumerate(evals):
        t, lam = d["t"][b, k], d["lam"][b, k]
        tmin = nsc.COLD_TMIN if mode == "cold" else nsc.WARM_TMIN
        np.testing.assert_allclose(t, np.maximum(e["g"], tmin), rtol=1e-12, atol=1e-12)
        lam_rule = mu / t if mode == "cold" else np.maximum(lam_w[min(k + 1, N - 1)], mu / t)
        np.testing.assert_allclose(lam, lam_rule, rtol=1e-11, atol=0)
        rg = e["g"] - t
        Q = e["H"] + e["Jg"].T @ np.diag(lam / t) @ e["Jg"]
        q0 = e["gf"] + e["Jg"].T @ (lam * rg / t)
        q1 = e["Jg"].T @ (1.0 / t)
        np.testing.assert_allclose(d["Q"][b, k], Q, rtol=1e-11, atol=1e-11 * max(1.0, np.abs(Q).max()))
        np.testing.assert_allclose(d["q0"][b, k], q0, rtol=1e-11, atol=1e-11 * max(1.0, np.abs(q0).max()))
        np.testing.assert_allclose(d["q1"][b, k], q1, rtol=1e-11, atol=1e-11 * max(1.0, np.abs(q1).max()))
        if k < N - 1:
            np.testing.assert_allclose(d["rc"][b, k], e["xnext"] - evals[k + 1]["z"][:nx], rtol=0, atol=1e-13)


@pytest.mark.parametrize("mode", nsc.MODES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_step_matches_dense_kkt(rt, case, mode, monkeypatch):
    path, name, kw, env, fused, copies = case
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)   # (read once, at rmpc_create)
    nd = DISTINCT[copies]
    sc, o, xinit, x0, params, duals = rt["inputs"](name, mode, nd, tuple(sorted(kw.items())))
    tile = lambda a: np.tile(a, (copies,) + (1,) * (a.ndim - 1))
    B = nd * copies
    s = rt["Solver"](sc.desc, max_batch=B)
    assert s.is_fused() == fused
    d = s.debug_step(tile(xinit), tile(x0), tile(params), None if duals is None else tuple(tile(a) for a in duals))
    s.close()
    assert d["t"].shape[2] == o.m
    # the switches selected the path this case is about (read at rmpc_create: a renamed or unread one would re-test the default)
    for key, want in PATHS[path].items():
        assert d["path"][key] == want, (key, d["path"])
    view = rt["spec_for"](sc.desc)   # ("" when the library holds no generated view of this model)
    assert path != "nospec" or view != ""
    assert d["path"]["generated_view"] == (view != "" and path != "nospec")
    assert np.all(d["ok"])
    if copies > 1:
        for key in ("Q", "q0", "q1", "rc", "t", "lam", "mu", "dz", "nu"):
            a = d[key].reshape(copies, nd, -1)
            assert np.array_equal(a, np.broadcast_to(a[0:1], a.shape)), key
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
    nsc.check_class("%s %s" % (_id(case), mode), errs, yard)
