"""The oracle's Newton step (Oracle.debug_step: first pass, then riccati()) against the refined dense KKT solution of
the same condensed QP, for every (config, horizon, mode) class of the GPU step tests (test_gpu_newton_step.py).  The
oracle is what the GPU parity tests compare converged plans with; this is what pins its step computation itself.
Bound and modes: newton_step_cases.py.  No GPU needed."""
import numpy as np
import pytest

import kkt_reference as ref
import newton_step_cases as nsc

B = 6

# (config, scenario overrides): every class of the GPU matrix
CLASSES = (
    [("cfg2", {}), ("chain2", {})]
    + [(n, {"time_horizon": N}) for n in ("cfg2", "chain2") for N in (1, 2, 5, 31, 32)]
    + [("cfg2", {"slack": True})] + [("cfg2", {"slack": True, "time_horizon": N}) for N in (1, 2, 5, 31, 32)]
    + [("cfg3", {}), ("boxer", {}), ("wc_boxer_slack", {})]
    + [("cfg4", {}), ("chain5", {}), ("chain6", {})] + [("cfg4", {"time_horizon": N}) for N in (12, 17, 21, 22, 30)]
    + [("chain4", {}), ("chain8", {}), ("wc_panda", {})]
    + [("cfg2", {"time_horizon": 40}), ("cfg4", {"time_horizon": 40})]
)


def _id(c):
    return c[0] + "".join("-%s%s" % (k[0], v) for k, v in sorted(c[1].items()))


@pytest.fixture(scope="module")
def rt(oracle_lib):
    from robot_mpcs_amd.scenarios import make_scenario
    return dict(Oracle=oracle_lib.Oracle, make_scenario=make_scenario)


@pytest.mark.parametrize("mode", nsc.MODES)
@pytest.mark.parametrize("cls", CLASSES, ids=_id)
def test_oracle_step_matches_dense_kkt(rt, cls, mode):
    name, kw = cls
    sc, o, xinit, x0, params, duals = nsc.make_inputs(rt["make_scenario"], rt["Oracle"], name, mode, B, **kw)
    errs, yard = [], []
    for b in range(B):
        d = o.debug_step(xinit[b], x0[b], params[b], None if duals is None else (duals[0][b], duals[1][b], duals[2][b]))
        assert d["ok"]
        assert d["mu"] == (sc.desc["options"]["mu0"] if mode == "cold" else nsc.WARM_MU_MIN)
        dz_ref, nu_ref, e_text, rel = nsc.reference_and_yardstick(d["Q"], d["q"], d["A"], d["B"], d["rc"])
        assert rel < ref.REFINE_TOL
        errs.append(ref.block_errors(d["dz"], d["nu"], dz_ref, nu_ref, o.nx))
        yard.append(e_text)
        if mode == "cold":
            evals, z = nsc.stage_evals(o, xinit[b], x0[b], params[b])
            nsc.check_descent(ref.merit_slope(evals, z, d["t"], d["mu"], d["dz"], dz_ref), d["dz"])
    nsc.check_class("oracle %s %s" % (_id(cls), mode), errs, yard)


def test_reference_detects_a_perturbed_dynamics_entry(rt):
    """Sensitivity of the measure itself: a relative error of 1e-6 in one entry of one stage's B moves the textbook step
    by far more than the bound allows, in a cold class."""
    sc, o, xinit, x0, params, _ = nsc.make_inputs(rt["make_scenario"], rt["Oracle"], "cfg2", "cold", 1)
    d = o.debug_step(xinit[0], x0[0], params[0])
    dz_ref, nu_ref, e_text, _ = nsc.reference_and_yardstick(d["Q"], d["q"], d["A"], d["B"], d["rc"])
    Bp = d["B"].copy()
    Bp[o.N // 2, 0, 0] *= 1.0 + 1e-6
    dz_p, nu_p = ref.textbook_riccati(d["Q"], d["q"], d["A"], Bp, d["rc"])
    assert ref.block_errors(dz_p, nu_p, dz_ref, nu_ref, o.nx) > 1e3 * ref.TOL_FACTOR * e_text


@pytest.mark.parametrize("name", ["cfg2", "cfg3", "cfg4"])
def test_descent_check_rejects_wrong_steps(rt, name):
    """The descent check itself: the oracle's step passes; the negated step, and the step whose states do not follow
    from its controls (the states of one stage zeroed: the linearised dynamics stay open), do not."""
    sc, o, xinit, x0, params, _ = nsc.make_inputs(rt["make_scenario"], rt["Oracle"], name, "cold", 2)
    for b in range(2):
        d = o.debug_step(xinit[b], x0[b], params[b])
        dz_ref, _, _ = ref.refined_solve(d["Q"], d["q"], d["A"], d["B"], d["rc"])
        evals, z = nsc.stage_evals(o, xinit[b], x0[b], params[b])
        good = ref.merit_slope(evals, z, d["t"], d["mu"], d["dz"], dz_ref)
        nsc.check_descent(good, d["dz"])
        assert ref.merit_slope(evals, z, d["t"], d["mu"], -d["dz"], dz_ref) > 0.0
        broken = d["dz"].copy()
        broken[o.N // 2, :o.nx] = 0.0
        assert ref.merit_slope(evals, z, d["t"], d["mu"], broken, dz_ref) > good
