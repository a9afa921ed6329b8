"""Cases and checks shared by the exact-Hessian tests (test_exact_hessian_cpu.py, test_gpu_exact_hessian.py): a solver
path's curvature terms C (what its recursion subtracts from the Gauss-Newton block per unit weight) and the Newton step
and verdict of the recursion on  H = Q - cw C.

Inputs: newton_step_cases.make_inputs in the modes `cold` and `conv`, B = 4 distinct instances per class.  The costate
a stage's dynamics term is weighted with is the one the first pass holds: zero in a cold pass, the stored costates
shifted like the plan in a warm one (stage k reads the costate of its successor k + 1, which starts from stage k + 2 of
the previous solve, the last one repeated).

Checks (the figures: DESIGN.md 6.1)
  (a) C against the oracle's C at the project's block tolerance, 1e-11 max(1, |C|_inf) per stage.
  (b) C against C_ref = H_GN - H_ref (hessian_reference.py), per stage:  |C - C_ref|_max <= u + REL * scale,  u the
      reference's own uncertainty, scale the max-norm of H_ref over the curved variables floored at 1.  REL is 8 times
      the worst  |C_oracle - C_ref|_max / scale  measured over every class and both modes by test_exact_hessian_cpu.py
      (1.12e-10, cfg2 at N = 32, conv): one analytic formula evaluated in two orders against a differencing error; a
      wrong term sits at 1e-1 of the scale or more.
  (c) with the reference verdict of  H = Q - cw C  (kkt_reference.verdict: per stage the smallest eigenvalue of the
      control block over its largest diagonal entry, the block scaled to a unit diagonal first -- unscaled, the slack's
      weight of 2e10 puts that ratio at 1e-12 for every instance of cfg3 and wc_boxer_slack, definite or not, and the
      multipliers of a converged plan put it at 1e-6; a Cholesky pivot is measured against its own diagonal entry): an
      instance is *clear* when the magnitude of the ratio exceeds CLEAR, *kept* when clear and positive definite.  Kept: ok == 1, dz and nu+ against
      the refined dense solve under newton_step_cases.check_class, a descent direction in the cold mode.  Clear and
      not positive definite: ok == 0, nothing else compared.  Every conv instance is kept, every cold class keeps at
      least a third, at most one instance of a class is unclear.
"""
import numpy as np

import hessian_reference as href
import kkt_reference as ref
import newton_step_cases as nsc

B = 4
MODES = ("cold", "conv")
CLEAR = 1e-6
REL_MEASURED = 1.12e-10  # worst |C_oracle - C_ref|_max / scale over the classes below (test_exact_hessian_cpu.py prints them)
REL = 8.0 * REL_MEASURED
H = lambda N: {"time_horizon": N}

# (config, scenario overrides) -> draw of the class: 0 unless the first draw misses a condition of (c) on the oracle
SALT = {("cfg3", ()): 4, ("boxer", ()): 4,   # (the first draw keeps one cold instance of four in both)
        ("aff3g", ()): 1}                    # (chain_cases.py; the same)


def key_of(name, kw):
    return (name, tuple(sorted(dict(kw).items())))


def class_id(name, kw):
    return name + "".join("-%s%s" % (k[0], v) for k, v in sorted(kw.items()))


def make_inputs(make_scenario, Oracle, name, mode, kw):
    """newton_step_cases.make_inputs for the class (name, kw).  The entry "mu0" of kw is no scenario override: it replaces
    the solver option of that name in the descriptor (the scene is the one of the class without it)."""
    kw = dict(kw)
    mu0 = kw.pop("mu0", None)

    def scenario(*a, **k):
        sc = make_scenario(*a, **k)
        if mu0 is not None:
            sc.desc["options"] = dict(sc.desc["options"], mu0=mu0)
        return sc

    return nsc.make_inputs(scenario, Oracle, name, mode, B, salt=SALT.get(key_of(name, kw), 0), **kw)


def consumed_costates(o, mode, duals, b):
    """nu+ of every stage as the first pass holds it: [N, nx] (row k weights the dynamics of stage k; row N - 1 unused)."""
    N = o.N
    out = np.zeros((N, o.nx))
    if mode != "cold":
        for k in range(N - 1):
            out[k] = duals[1][b][min(k + 2, N - 1)]
    return out


def instance_reference(o, mode, xinit, x0, params, duals, b):
    """Everything of instance b that does not depend on the path under test: the oracle's hook output at cw = 0 (blocks,
    t, lam, C), the stage evaluations and the difference reference of every stage (C_ref, scale, u)."""
    dl = None if duals is None else (duals[0][b], duals[1][b], duals[2][b])
    d = o.debug_step(xinit[b], x0[b], params[b], dl, curv=0.0)
    evals, z = nsc.stage_evals(o, xinit[b], x0[b], params[b])
    P = params[b].reshape(o.N, o.npar)
    nun = consumed_costates(o, mode, duals, b)
    Cref = np.zeros_like(d["C"]); scale = np.zeros(o.N); u = np.zeros(o.N)
    for k in range(o.N):
        Cref[k], Hk, u[k] = href.curvature_reference(o, z[k], P[k], d["lam"][k], nun[k] if k < o.N - 1 else None, k == 0)
        scale[k] = href.hessian_scale(o, Hk)
    return dict(orc=d, evals=evals, z=z, Cref=Cref, scale=scale, u=u)


def check_against_oracle(label, C, C_orc):
    """(a)"""
    for k in range(C.shape[0]):
        tol = 1e-11 * max(1.0, float(np.abs(C_orc[k]).max()))
        np.testing.assert_allclose(C[k], C_orc[k], rtol=0, atol=tol, err_msg="%s stage %d" % (label, k))


def reference_figure(C, r):
    """Worst |C - C_ref|_max / scale over the stages, and whether every stage keeps the bound of (b)."""
    worst, ok = 0.0, True
    for k in range(C.shape[0]):
        err = float(np.abs(C[k] - r["Cref"][k]).max())
        worst = max(worst, err / r["scale"][k])
        ok = ok and err <= r["u"][k] + REL * r["scale"][k]
    return worst, ok


def check_against_reference(label, C, r):
    """(b)"""
    worst, ok = reference_figure(C, r)
    assert ok, "%s: |C - C_ref| / scale = %.3e (bound: u + %.1e; u up to %.1e)" % (label, worst, REL, r["u"].max())
    return worst


def classify(Q, C, cw, A, Bm):
    """(pd, ratio, clear, kept) of H = Q - cw C."""
    nx = A.shape[1]
    pd, ratio = ref.verdict(Q - cw * C, A, Bm, gn_diag=np.array([np.diag(Qk)[nx:] for Qk in Q]))
    clear = abs(ratio) > CLEAR
    return pd, ratio, clear, clear and pd


def check_steps(label, mode, o, cw, insts, nu_from):
    """(c).  insts: per instance dict(Q, C, q, A, B, rc, t, mu, dz, nu, ok, evals, z) -- blocks as the path returned them."""
    errs, yard, kept, unclear = [], [], 0, 0
    for b, s in enumerate(insts):
        pd, ratio, clear, keep = classify(s["Q"], s["C"], cw, s["A"], s["B"])
        print("exact-hessian %s inst %d: pd %d ratio %.3e ok %d" % (label, b, pd, ratio, s["ok"]))
        if not clear:
            unclear += 1
            continue
        assert bool(s["ok"]) == pd, (label, b, ratio, s["ok"])
        if not keep:
            continue
        kept += 1
        Hm = s["Q"] - cw * s["C"]
        dz_ref, nu_ref, e_text, rel = nsc.reference_and_yardstick(Hm, s["q"], s["A"], s["B"], s["rc"])
        assert rel < ref.REFINE_TOL
        errs.append(ref.block_errors(s["dz"], s["nu"], dz_ref, nu_ref, o.nx, nu_from=nu_from))
        yard.append(e_text)
        if mode == "cold":
            nsc.check_descent(ref.merit_slope(s["evals"], s["z"], s["t"], s["mu"], s["dz"], dz_ref), s["dz"])
    n = len(insts)
    assert unclear <= 1, (label, unclear)
    if mode == "conv":
        assert kept == n, (label, kept, n)
    else:
        assert 3 * kept >= n, (label, kept, n)
    nsc.check_class("exact-hessian %s" % label, errs, yard)
    return kept, unclear
