"""The oracle's curvature terms and its step on the exact Hessian (Oracle.debug_step(curv=cw): C and the recursion on
Q - cw C), for every (config, horizon, weight) class of test_gpu_exact_hessian.py in the modes cold and conv:
C against the difference reference of hessian_reference.py -- on the diff-drive configs the first check of dd_dyn_curv
and of the frame-rotation term at all --, and the step and the recursion's verdict against kkt_reference.  The bound of
the reference check is fixed here: the test prints the worst |C - C_ref| / scale of every class, and
exact_hessian_cases.REL is 8 times the worst of them.  Checks and bound: exact_hessian_cases.py.  No GPU needed.

Measured (|C_oracle - C_ref|_max / scale, worst stage and instance of the class; u: the reference's own uncertainty):
  point robots   cold at most 1.1e-11, conv 4.7e-11 (cfg2), 8.9e-11 (chain2), 1.12e-10 (cfg2 N = 32); u up to 2.4e-9
  diff-drive     cfg3, boxer, wc_boxer_slack, boxer N = 2: cold at most 5.2e-12, conv at most 9.8e-12; u up to 8.0e-11
  arms           cfg4, chain4, chain5, chain6, chain8, wc_panda: cold at most 1.9e-12, conv at most 7.2e-11; u up to 1.1e-11
The worst of them, 1.12e-10, times 8 is exact_hessian_cases.REL.  Of the 88 cold instances 12 are not positive definite
(the oracle returns ok = 0 for each), every conv instance is; no instance is unclear.
"""
import functools

import numpy as np
import pytest

import exact_hessian_cases as ehc

H = ehc.H
# (config, scenario overrides, curvature weight)
CLASSES = (
    [(n, kw, 1.0) for n in ("cfg2", "chain2") for kw in ({}, H(1), H(2), H(32))]
    + [(n, {}, 0.5) for n in ("cfg2", "chain2")]
    + [(n, {}, 1.0) for n in ("cfg3", "boxer", "wc_boxer_slack")] + [("boxer", H(2), 1.0)]
    + [(n, {}, 1.0) for n in ("cfg4", "chain5", "chain6", "chain4", "chain8", "wc_panda")]
    + [("cfg2", {"slack": True}, 1.0)]
    + [("cfg2", {"mu0": 1e-2}, 1.0)]   # (the cold class of the lane-per-instance recursion: test_gpu_exact_hessian.py)
)
DIFFDRIVE = ("cfg3", "boxer", "wc_boxer_slack")


def _id(c):
    return ehc.class_id(c[0], c[1]) + ("" if c[2] == 1.0 else "-cw%g" % c[2])


@pytest.fixture(scope="module")
def rt(oracle_lib):
    from robot_mpcs_amd.scenarios import make_scenario

    @functools.lru_cache(maxsize=None)
    def prepared(name, mode, kw):
        sc, o, xinit, x0, params, duals = ehc.make_inputs(make_scenario, oracle_lib.Oracle, name, mode, kw)
        refs = [ehc.instance_reference(o, mode, xinit, x0, params, duals, b) for b in range(ehc.B)]
        return sc, o, xinit, x0, params, duals, refs

    return dict(prepared=prepared)


@pytest.mark.parametrize("mode", ehc.MODES)
@pytest.mark.parametrize("cls", CLASSES, ids=_id)
def test_oracle_exact_hessian_step(rt, cls, mode):
    name, kw, cw = cls
    sc, o, xinit, x0, params, duals, refs = rt["prepared"](name, mode, tuple(sorted(kw.items())))
    label = "oracle %s %s" % (_id(cls), mode)
    insts, worst = [], 0.0
    for b, r in enumerate(refs):
        dl = None if duals is None else (duals[0][b], duals[1][b], duals[2][b])
        d = o.debug_step(xinit[b], x0[b], params[b], dl, curv=cw)
        g = r["orc"]
        # the weight changes the step and nothing else of the hook's output
        for key in ("Q", "C", "q", "A", "B", "rc", "t", "lam"):
            assert np.array_equal(d[key], g[key]), key
        assert np.array_equal(d["C"], np.transpose(d["C"], (0, 2, 1)))
        if kw.get("slack"):
            assert not np.any(d["C"])
            assert np.array_equal(d["dz"], g["dz"]) and np.array_equal(d["nu"], g["nu"]) and d["ok"] == g["ok"]
        if o.N == 2:   # stage N - 1 carries no dynamics term: nothing outside the q block
            assert not np.any(d["C"][o.N - 1][o.n:, :]) and not np.any(d["C"][o.N - 1][:, o.n:])
        if not kw.get("slack"):   # (a model without terms: C = 0 is no statement about its exact Hessian)
            worst = max(worst, ehc.check_against_reference("%s inst %d" % (label, b), d["C"], r))   # (d) on the diff-drive configs
        insts.append(dict(Q=d["Q"], C=d["C"], q=d["q"], A=d["A"], B=d["B"], rc=d["rc"], t=d["t"], mu=d["mu"], dz=d["dz"],
                          nu=d["nu"], ok=d["ok"], evals=r["evals"], z=r["z"]))
    print("exact-hessian %s: |C - C_ref| / scale %.3e (u up to %.1e)" % (label, worst, max(r["u"].max() for r in refs)))
    ehc.check_steps(label, mode, o, cw, insts, nu_from=0)


def test_diffdrive_classes_have_dynamics_curvature(rt):
    """The conv inputs of the diff-drive configs do exercise nu . grad^2 Phi: entries outside the q block at 1e-3 of the
    stage's scale or more (a reference that saw zeros there would check nothing of dd_dyn_curv)."""
    for name in DIFFDRIVE:
        sc, o, xinit, x0, params, duals, refs = rt["prepared"](name, "conv", ())
        big = 0.0
        for r in refs:
            for k in range(o.N - 1):
                Ck = r["Cref"][k].copy()
                Ck[:o.n, :o.n] = 0.0
                big = max(big, float(np.abs(Ck).max()) / r["scale"][k])
        assert big > 1e-3, (name, big)


def test_reference_detects_wrong_terms(rt):
    """Sensitivity of check (b): one negated dynamics entry, two swapped ones and a dropped (theta, theta) term of the
    oracle's C are far outside the bound."""
    sc, o, xinit, x0, params, duals, refs = rt["prepared"]("boxer", "conv", ())
    iu = o.nx + o.ns
    hits = 0
    for r in refs:
        C = r["orc"]["C"]
        assert ehc.reference_figure(C, r)[1]
        for mutate in ("negate", "swap", "drop"):
            Cm = C.copy()
            for k in range(o.N - 1):
                if mutate == "negate":
                    Cm[k][2, 6] = Cm[k][6, 2] = -C[k][2, 6]
                elif mutate == "swap":
                    Cm[k][2, 6] = Cm[k][6, 2] = C[k][7, iu]
                    Cm[k][7, iu] = Cm[k][iu, 7] = C[k][2, 6]
                else:
                    Cm[k][2, 2] = 0.0
            hits += not ehc.reference_figure(Cm, r)[1]
    assert hits == 3 * len(refs)
