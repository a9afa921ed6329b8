"""Cases and checks shared by the Newton-step tests (test_newton_step_cpu.py, test_gpu_newton_step.py): the inputs of
a (config, mode) class, the dense reference of an instance and the bound a solver path has to keep.

Modes
  cold  what ``make_scenario`` delivers: the first pass of a cold solve (mu0, slacks clamped at 1e-2).
  late  x0 is the oracle's converged plan of the same scenario, the duals are that solve's with the multipliers of the
        rows at the warm-start clamp (t = 1e-4) and of a random third of the others set to 10^U(0, 4), and the stored
        barrier parameter (1e-10) makes the warm start begin at its floor 1e-6: the blocks of a late iteration
        (lam / t up to 1e8) through the existing warm first pass.
  conv  (the exact-Hessian tests only: not in MODES) x0 is the oracle's converged plan and the duals are that solve's
        own, unmodified, with a stored barrier parameter of 1e-10: the blocks a late iteration really sees.  The random
        multipliers of `late` on convex distance rows make the exact Hessian indefinite by construction.

Tolerance: errors are measured per stage and block against the refined dense solution (kkt_reference.block_errors);
the textbook fp64 Riccati recursion's worst error over the instances of the class is the unit, and a solver path may
be TOL_FACTOR = 16 times that -- differently ordered but equally stable eliminations of one system differ by small
multiples of one bound, a wrong term sits orders of magnitude away.
"""
import zlib

import numpy as np

import kkt_reference as ref

WARM_TMIN = 1e-4     # kWarmTMin / ORC_WARM_TMIN
WARM_MU_MIN = 1e-6   # kWarmMuMin / ORC_WARM_MU_MIN
COLD_TMIN = 1e-2     # kTMin / ORC_TMIN
MODES = ("cold", "late")


def case_seed(*key):
    return zlib.crc32(repr(key).encode()) % 100000


def make_inputs(make_scenario, Oracle, name, mode, B, salt=0, **kw):
    """Scenario, oracle and the inputs of the step hooks: xinit, x0, params, duals (None in the cold mode).  salt: another
    draw of the same class."""
    assert mode in ("cold", "late", "conv"), mode
    seed = case_seed(name, sorted(kw.items())) + salt
    sc = make_scenario(name, B=B, seed=seed, **kw)
    o = Oracle(sc.desc)
    if mode == "cold":
        return sc, o, sc.xinit, sc.x0, sc.params, None
    rng = np.random.default_rng(seed + 1)
    N, m, nx = o.N, o.m, o.nx
    x0 = np.zeros((B, N, o.nv)); lam = np.zeros((B, N, m)); nu = np.zeros((B, N, nx))
    clamped = 0
    for b in range(B):
        r = o.solve_warm(sc.xinit[b], sc.x0[b], sc.params[b])
        assert r["exitflag"] in (1, 2), (name, b, r["exitflag"])
        x0[b] = r["z"]
        lam[b], nu[b] = r["duals"][0], r["duals"][1]
        if mode == "conv":
            continue
        P = sc.params[b].reshape(N, o.npar)
        for k in range(N):
            g = o.eval_stage(x0[b, k], P[k], derivs=False, dynamics=False, fixed_state=(k == 0))["g"]
            ks = min(k + 1, N - 1)   # (stage k starts from the multipliers of stage k + 1)
            big = (g < WARM_TMIN) | (rng.random(m) < 1.0 / 3.0)
            clamped += int((g < WARM_TMIN).sum())
            lam[b, ks] = np.where(big, 10.0 ** rng.uniform(0.0, 4.0, m), lam[b, ks])
    # (one or two stages with the first state fixed: the converged plan of the point robots touches no row)
    assert mode == "conv" or clamped > 0 or N <= 2, "no row of the class sits at the warm-start clamp"
    return sc, o, sc.xinit, x0, sc.params, (lam, nu, np.full(B, 1e-10))


def stage_evals(o, xinit, x0, params):
    """Oracle.eval_stage of every stage of one instance (stage 0 at xinit)."""
    N = o.N
    P = params.reshape(N, o.npar)
    z = np.array(x0, dtype=np.float64).reshape(N, o.nv)
    z[0, :o.nx] = xinit
    return [o.eval_stage(z[k], P[k], fixed_state=(k == 0)) for k in range(N)], z


def dynamics_blocks(evals):
    return np.array([e["A"] for e in evals]), np.array([e["B"] for e in evals])


def reference_and_yardstick(Q, q, A, B, rc):
    """Refined dense solution of one instance and the textbook recursion's error against it."""
    dz_ref, nu_ref, rel = ref.refined_solve(Q, q, A, B, rc)
    nx = A.shape[1]
    dz_t, nu_t = ref.textbook_riccati(Q, q, A, B, rc)
    return dz_ref, nu_ref, ref.block_errors(dz_t, nu_t, dz_ref, nu_ref, nx), rel


def check_class(label, errs, yard):
    """errs / yard: per-instance errors of the path under test and of the textbook recursion.  Prints the figures, then
    asserts the bound; returns the ratio (path over textbook, worst of the class)."""
    unit = max(yard)
    worst = max(errs)
    ratio = worst / unit if unit > 0.0 else (0.0 if worst == 0.0 else np.inf)
    print("newton-step %s: path %.3e textbook %.3e ratio %.2f" % (label, worst, unit, ratio))
    assert worst <= ref.TOL_FACTOR * unit, (label, worst, unit, ratio)
    return ratio


def check_descent(slope, dz):
    """Cold classes: the step is a descent direction of the solver's merit (kkt_reference.merit_slope).  The slope is zero
    only for a zero step: a single stage whose state is fixed, zero inputs at the analytic centre of symmetric input
    limits (the point robot at N = 1), where the Newton step is exactly zero."""
    assert slope < 0.0 or (slope == 0.0 and not np.any(dz)), slope
