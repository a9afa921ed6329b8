"""Reference for the Newton step of one interior-point iteration (tests only).

The condensed QP of an iteration is

    min  sum_k  1/2 dz_k^T Q_k dz_k + q_k^T dz_k
    s.t. dx_0 = 0,   dx_{k+1} = A_k dx_k + B_k dw_k + rc_k        (dz_k = [dx_k | dw_k])

``refined_solve`` assembles its full KKT matrix (unknowns dz_0 .. dz_{N-1} and one costate block per stage, the
fixed initial state being a constraint), factors it once with partial pivoting and refines the solution with
residuals in ``numpy.longdouble``.  ``textbook_riccati`` is a plain fp64 Riccati recursion in gain form; it is neither
the oracle nor a port of a kernel path: its error against the refined solution is the yardstick the solver paths are
measured with (``block_errors``, ``TOL_FACTOR``).
"""
import numpy as np
import scipy.linalg

LD = np.longdouble
REFINE_TOL = 1e-18   # last correction over the solution's max-norm, for the result to count as the reference
TOL_FACTOR = 16.0    # a solver path may be this many times the textbook recursion's worst error of its class


def kkt_system(Q, q, A, B, rc):
    """Q [N, nv, nv], q [N, nv], A [N, nx, nx], B [N, nx, nw], rc [N, nx] (stage N-1 of A, B, rc unused).
    Returns K, r with K y = r, y = [dz_0 .. dz_{N-1} | nu_0 .. nu_{N-1}]; nu_k is the costate of the constraint
    that fixes dx_k (nu_0: the initial state), with the sign that makes nu_k = P_k dx_k + p_k."""
    N, nv = q.shape
    nx = A.shape[1]
    n, m = N * nv, N * nx
    K = np.zeros((n + m, n + m)); r = np.zeros(n + m)
    for k in range(N):
        K[k * nv:(k + 1) * nv, k * nv:(k + 1) * nv] = Q[k]
        r[k * nv:(k + 1) * nv] = -q[k]
    K[n:n + nx, 0:nx] = -np.eye(nx)
    for k in range(N - 1):
        R = slice(n + (k + 1) * nx, n + (k + 2) * nx)
        K[R, k * nv:k * nv + nx] = A[k]
        K[R, k * nv + nx:(k + 1) * nv] = B[k]
        K[R, (k + 1) * nv:(k + 1) * nv + nx] = -np.eye(nx)
        r[R] = -rc[k]
    K[:n, n:] = K[n:, :n].T
    return K, r


def refined_solve(Q, q, A, B, rc, max_iter=12):
    """(dz [N, nv], nu [N, nx]) in longdouble, and the last correction over the solution's max-norm.  Raises when the
    correction does not get below REFINE_TOL: a case without a reference is an error, never a case dropped."""
    N, nv = q.shape
    nx = A.shape[1]
    K, r = kkt_system(Q, q, A, B, rc)
    lu = scipy.linalg.lu_factor(K)
    Kl, rl = K.astype(LD), r.astype(LD)
    y = scipy.linalg.lu_solve(lu, r).astype(LD)
    rel = np.inf
    for _ in range(max_iter):
        d = scipy.linalg.lu_solve(lu, np.asarray(rl - Kl @ y, dtype=np.float64))
        y = y + d
        rel = float(np.abs(d).max() / np.abs(y).max())
        if rel < REFINE_TOL:
            break
    if not rel < REFINE_TOL:
        raise AssertionError("iterative refinement stalled at %.2e (cond %.1e)" % (rel, np.linalg.cond(K)))
    n = N * nv
    return y[:n].reshape(N, nv), y[n:].reshape(N, nx), rel


def textbook_riccati(Q, q, A, B, rc):
    """fp64 Riccati recursion in gain form with a symmetrised cost-to-go: (dz, nu)."""
    N, nv = q.shape
    nx = A.shape[1]
    P = np.zeros((nx, nx)); p = np.zeros(nx)
    Ks, ks, Ps, ps = [None] * N, [None] * N, [None] * N, [None] * N
    for k in range(N - 1, -1, -1):
        Qk, qk = Q[k].copy(), q[k].copy()
        if k < N - 1:
            AB = np.hstack([A[k], B[k]])
            Qk += AB.T @ P @ AB
            qk += AB.T @ (P @ rc[k] + p)
        Qxx, Qxu, Quu = Qk[:nx, :nx], Qk[:nx, nx:], Qk[nx:, nx:]
        c = scipy.linalg.cho_factor(Quu)
        Ks[k] = -scipy.linalg.cho_solve(c, Qxu.T)
        ks[k] = -scipy.linalg.cho_solve(c, qk[nx:])
        P = Qxx + Qxu @ Ks[k]
        P = 0.5 * (P + P.T)
        p = qk[:nx] + Qxu @ ks[k]
        Ps[k], ps[k] = P, p
    dz = np.zeros((N, nv)); nu = np.zeros((N, nx)); dx = np.zeros(nx)
    for k in range(N):
        du = Ks[k] @ dx + ks[k]
        dz[k, :nx] = dx; dz[k, nx:] = du
        nu[k] = Ps[k] @ dx + ps[k]
        if k < N - 1:
            dx = A[k] @ dx + B[k] @ du + rc[k]
    return dz, nu


def verdict(Q, A, B, gn_diag=None):
    """Is the condensed QP's reduced Hessian positive definite, and by what margin?  The textbook recursion on the
    cost-to-go alone, never raising: per stage (last to first) the smallest eigenvalue of the control block
    Quu = Q_uu + B^T P B over its largest diagonal entry, the block first scaled to a unit diagonal, S Quu S with
    S = diag(d)^-1/2 (what a Cholesky pivot is measured against is its own diagonal entry, and without the scaling the
    slack's weight, 2e10 beside input weights of 1e-2, would make the ratio 1e-12 for every block of a model with a
    slack, definite or not; with equal diagonal entries the two ratios are the same number).  d_i = |Quu_ii|, and no
    less than gn_diag[k, i] where that is given -- the diagonal of the Gauss-Newton control block Q is made from, so
    that an entry the curvature terms have cancelled or turned negative is measured against what it was made of.
    Returns (pd, ratio): all stages positive -> (True, the smallest ratio); else (False, the ratio of the first stage
    met that is not positive -- the recursion below it is undefined)."""
    N = Q.shape[0]
    nx = A.shape[1]
    P = np.zeros((nx, nx))
    worst = np.inf
    for k in range(N - 1, -1, -1):
        Qk = np.array(Q[k], dtype=np.float64)
        if k < N - 1:
            AB = np.hstack([A[k], B[k]])
            Qk = Qk + AB.T @ P @ AB
        Qxx, Qxu, Quu = Qk[:nx, :nx], Qk[:nx, nx:], Qk[nx:, nx:]
        Quu = 0.5 * (Quu + Quu.T)
        d = np.abs(np.diag(Quu))
        if gn_diag is not None:
            d = np.maximum(d, gn_diag[k])
        s = 1.0 / np.sqrt(np.where(d > 0.0, d, 1.0))
        ratio = float(np.linalg.eigvalsh(Quu * s[:, None] * s[None, :])[0])
        if not ratio > 0.0:
            return False, ratio
        worst = min(worst, ratio)
        P = Qxx - Qxu @ np.linalg.solve(Quu, Qxu.T)
        P = 0.5 * (P + P.T)
    return True, worst


def block_errors(dz, nu, dz_ref, nu_ref, nx, nu_from=0):
    """Worst error over the stages and the three blocks of a stage (dx, the controls with the slack, nu+): max-norm of
    the difference over the max-norm of that block of the reference.  A block of zeros is compared absolutely; the
    reference is known to REFINE_TOL of its own max-norm, so a block of it below that is a block of zeros (the dense
    solve leaves 1e-2x there where the recursions return an exact 0).  nu_from: first stage whose nu+ is compared."""
    worst = 0.0
    floor = REFINE_TOL * max(float(np.abs(dz_ref).max()), float(np.abs(nu_ref).max()))
    for k in range(dz_ref.shape[0]):
        blocks = [(dz[k, :nx], dz_ref[k, :nx]), (dz[k, nx:], dz_ref[k, nx:])] + ([(nu[k], nu_ref[k])] if k >= nu_from else [])
        for got, ref in blocks:
            scale = float(np.abs(ref).max())
            err = float(np.abs(got.astype(LD) - ref).max())
            if not np.isfinite(err):
                return np.inf
            worst = max(worst, err / scale if scale > floor else err)
    return worst


def merit_slope(evals, z, t, mu, dz, dz_rho):
    """Directional derivative along dz of the merit the solver's line search uses, phi = f - mu sum log t + rho theta,
    theta = |dynamics defects|_1 + |g - t|_1 (+ the fixed first state).  Both parts are formed from dz itself:
    gphi = sum_k gf.dz - mu sum dt / t with the slack step dt = g - t + Jg dz, and D theta through A, B and the defects --
    a defect r_k = f(z_k) - x_{k+1} changes by c_k = A dx_k + B dw_k - dx_{k+1}, which contributes sign(r_k) c_k (|c_k|
    where r_k = 0); a first state that moves contributes |dx_0|; the slack step closes g - t by its definition.  rho is
    fixed BEFORE the step is looked at, by the solver's rule (rho = gphi / (0.9 theta) + 1 when theta > 1e-13) applied to
    dz_rho, the refined reference step -- never to the step that is judged, for which the rule would make any direction
    a descent direction.  evals: Oracle.eval_stage of every stage at z [N, nv]."""
    nx = evals[0]["A"].shape[0]
    N = len(evals)

    def gphi_of(step):
        s = 0.0
        for k, e in enumerate(evals):
            dt = e["g"] - t[k] + e["Jg"] @ step[k]
            s += float(e["gf"] @ step[k] - mu * np.sum(dt / t[k]))
        return s

    theta = 0.0
    dtheta = float(np.abs(dz[0, :nx]).sum())
    for k, e in enumerate(evals):
        rg = np.abs(e["g"] - t[k]).sum()
        theta += float(rg)
        dtheta -= float(rg)
        if k < N - 1:
            r = e["xnext"] - z[k + 1, :nx]
            c = e["A"] @ dz[k, :nx] + e["B"] @ dz[k, nx:] - dz[k + 1, :nx]
            theta += float(np.abs(r).sum())
            dtheta += float(np.where(r != 0.0, np.sign(r) * c, np.abs(c)).sum())
    rho = max(0.0, gphi_of(np.asarray(dz_rho, dtype=np.float64)) / (0.9 * theta) + 1.0) if theta > 1e-13 else 0.0
    return gphi_of(dz) + rho * dtheta
