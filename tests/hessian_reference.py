"""Reference for the exact stage Hessian of one interior-point iteration (tests only).

The Lagrangian of stage k is  L_k(z) = f(z) - lam^T g(z) + nu+^T Phi(z)  (nu+: the costate of the stage's successor;
the last stage has no dynamics term), its gradient  gf - Jg^T lam + [A | B]^T nu+  is analytic in ``Oracle.eval_stage``.
``exact_hessian`` differentiates that gradient in all nvar variables by central differences at h, h/2 and h/4 and
extrapolates twice (Richardson: the error terms h^2 and h^4 cancel); it returns the value and its own uncertainty u,
the max-norm of the difference between the last two extrapolated values.  No second derivative of the oracle or of a
kernel enters.  ``curvature_reference`` is what a solver path has to subtract from its Gauss-Newton block per unit
weight:  C_ref = H_GN - H_ref  with H_GN the ``H`` of ``eval_stage`` (the constraints' Gauss-Newton part
Jg^T diag(lam / t) Jg is no part of either).
"""
import numpy as np

H0 = 1e-3   # largest step of the three


def lagrangian_gradient(o, z, p, lam, nu_next, fixed_state):
    """gf - Jg^T lam (+ [A | B]^T nu+ when nu_next is not None) at z."""
    e = o.eval_stage(z, p, dynamics=nu_next is not None, fixed_state=fixed_state)
    g = e["gf"] - e["Jg"].T @ lam
    if nu_next is not None:
        g = g + np.hstack([e["A"], e["B"]]).T @ nu_next
    return g


def _central(o, z, p, lam, nu_next, fixed_state, h):
    nv = z.size
    D = np.zeros((nv, nv))
    for j in range(nv):
        zp = z.copy(); zm = z.copy()
        zp[j] += h; zm[j] -= h
        D[:, j] = (lagrangian_gradient(o, zp, p, lam, nu_next, fixed_state)
                   - lagrangian_gradient(o, zm, p, lam, nu_next, fixed_state)) / (zp[j] - zm[j])
    return 0.5 * (D + D.T)


def exact_hessian(o, z, p, lam, nu_next, fixed_state, h=H0):
    """(H_ref [nv, nv], u): Hessian of the stage Lagrangian at z and its uncertainty (max-norm)."""
    z = np.array(z, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    d0, d1, d2 = (_central(o, z, p, lam, nu_next, fixed_state, h / s) for s in (1.0, 2.0, 4.0))
    r0 = (4.0 * d1 - d0) / 3.0
    r1 = (4.0 * d2 - d1) / 3.0
    r2 = (16.0 * r1 - r0) / 15.0
    return r2, float(np.abs(r2 - r1).max())


def curvature_reference(o, z, p, lam, nu_next, fixed_state, h=H0):
    """(C_ref, H_ref, u) of one stage; nu_next None: a stage without a dynamics term (stage N - 1)."""
    H_ref, u = exact_hessian(o, z, p, lam, nu_next, fixed_state, h)
    H_gn = o.eval_stage(z, p, dynamics=False, fixed_state=fixed_state)["H"]
    return H_gn - H_ref, H_ref, u


def curved_variables(o):
    """Indices of the variables the curvature terms live on: the q block and, for the unicycle, (theta, omega, u1, v, u0)."""
    idx = set(range(o.n))
    if o.d["robot"] == 1:   # RMPC_ROBOT_DIFFDRIVE
        iu = o.nx + o.ns
        idx |= {2, 7, iu + 1, 6, iu}
    return sorted(idx)


def hessian_scale(o, H_ref):
    """max-norm of H_ref over the curved variables, floored at 1 (the slack's weight stays out of it)."""
    idx = curved_variables(o)
    return max(1.0, float(np.abs(H_ref[np.ix_(idx, idx)]).max()))
