"""Constructed inputs of the steady-loop tests (tests/test_gpu_steady_loop.py runs them on the device,
tests/test_steady_loop_cpu.py checks on the CPU that they contain what they are meant to contain and that every
floating-point decision in them is far from its threshold).  Instances are constructed, not drawn: every property of
instance b is picked from a short table by b modulo a prime of its own, so that any two properties occur in every
combination within a few dozen instances and in mixed order inside a wavefront.  Only the cursors are drawn."""
import numpy as np

from steady_loop_reference import ROBOT_DIFFDRIVE, end_link

# arrival tolerance and rest speed of the fleet's loop (fleet.MixedFleetShard)
TOL = {"cfg2": 0.25, "cfg3": 0.35, "cfg4": 0.10}
SETTLE_VEL = {"cfg2": 0.02, "cfg3": 0.02, "cfg4": 0.03}

FLAGS = (1, 2, 0, -6, -7)                               # b % 5
JOINTS = ("lo-0.02", "lo-0.08", "hi+0.02", "hi+0.08", "in", "in", "in")   # b % 7
DIRS = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [0.6, 0.8, 0], [0, -0.6, 0.8], [-1.0, 0, 0], [0, 0.8, -0.6]])


def _inside(lim, k, salt):
    """(k, n) configurations inside the box: joint j of row i at one of eight fractions of the width, never closer than
    15 % to a limit"""
    lo, hi = lim
    n = lo.size
    frac = np.array([0.2, 0.65, 0.35, 0.8, 0.5, 0.15, 0.7, 0.45])
    i, j = np.meshgrid(np.arange(k), np.arange(n), indexing="ij")
    return lo + frac[(3 * i + 5 * j + salt) % 8] * (hi - lo)


def _speeds(desc, x, mult, settle_vel, b):
    """the speed entries of state x: one of them at mult x settle_vel (sign by b), the others at a tenth of that"""
    v = mult * settle_vel
    if desc["robot"] == ROBOT_DIFFDRIVE:
        x[3:6] = [0.3 + 0.001 * b, -0.2, 0.1]    # (entries the speed test must not look at: all above settle_vel)
        x[6], x[7] = (v, -0.1 * v) if b % 2 else (0.1 * v, -v)
    else:
        n = desc["n"]
        x[n:2 * n] = 0.1 * v
        x[n + b % n] = v if b % 4 < 2 else -v


def retarget_case(name, desc, lim, oracle, B, pool_len, seed=0, settle_min_dwell=4, max_dwell=9, fail_reset_after=3,
                  use_flags=True, use_failrun=True, use_limits=True):
    """One call's inputs for B instances of config ``name``: (state, args) as ``retarget_step`` takes them.  ``lim``
    (2, n): the joint-limit box.  ``use_*``: which of the optional arrays the call will be given -- a goal is placed
    relative to the state the distance will be taken from, which is the start state for an instance that is reset."""
    n, nx, N = desc["n"], desc["nx"], desc["N"]
    nvar = nx + desc["ns"] + desc["nu"]
    tol, sv = TOL[name], SETTLE_VEL[name]
    lo, hi = np.asarray(lim[0], dtype=np.float64), np.asarray(lim[1], dtype=np.float64)
    w = hi - lo
    rng = np.random.default_rng(seed)
    b_ = np.arange(B)
    xinit, x_start = np.zeros((B, nx)), np.zeros((B, nx))
    xinit[:, :n], x_start[:, :n] = _inside((lo, hi), B, 0), _inside((lo, hi), B, 3)
    exitflag = np.array([FLAGS[b % 5] for b in range(B)], dtype=np.int32)
    iters = (1 + (7 * b_) % 23).astype(np.int32)
    dw_tab = np.array([settle_min_dwell - 2, settle_min_dwell - 1, settle_min_dwell, max_dwell - 2, max_dwell - 1, max_dwell])
    dwell = dw_tab[np.array([0, 1, 2, 3, 4, 5, 0, 2, 4, 1, 3])[b_ % 11]].astype(np.int32)
    fr_tab = np.array([fail_reset_after - 2, fail_reset_after - 1, fail_reset_after, 0])
    failrun = np.maximum(fr_tab[np.array([0, 1, 2, 3, 1, 0, 2, 1, 3, 1, 0, 1, 2])[b_ % 13]], 0).astype(np.int32)
    goal = np.zeros((B, 3))
    for b in range(B):
        kind, j = JOINTS[b % 7], (b // 7) % n
        oob = kind in ("lo-0.08", "hi+0.08") and use_limits
        if kind != "in":
            off = float(kind[3:])
            xinit[b, j] = lo[j] - off * w[j] if kind[:2] == "lo" else hi[j] + off * w[j]
        _speeds(desc, xinit[b], 0.5 if b % 2 == 0 else 2.0, sv, b)
        _speeds(desc, x_start[b], 0.5 if b % 3 != 0 else 2.0, sv, b + 1)
        failed = use_flags and exitflag[b] < 0
        fr = (int(failrun[b]) if use_failrun else 0) + 1
        reset = oob or (failed and fail_reset_after > 0 and fr >= fail_reset_after)
        at = end_link(oracle, desc, x_start[b] if reset else xinit[b])
        goal[b] = at + (0.5 if b % 3 == 0 else 2.0) * tol * DIRS[b % 17 % 7]
    # distinct values everywhere else, so that a missing or a stray write shows
    x0 = 1000.0 + np.arange(B * N * nvar, dtype=np.float64).reshape(B, N, nvar) / 8.0
    pool = 50.0 + np.arange(B * pool_len * 3, dtype=np.float64).reshape(B, pool_len, 3) / 16.0
    cursor = (pool_len * rng.integers(0, 4, size=B) + rng.integers(-2, 2, size=B)).clip(0).astype(np.int32)
    state = dict(xinit=xinit, x0=x0, goal=goal, cursor=cursor, dwell=dwell, failrun=failrun if use_failrun else None,
                 exitflag=exitflag if use_flags else None, iters=iters)
    args = dict(oracle=oracle, desc=desc, pool=pool, x_start=x_start,
                lower=np.tile(lo, (B, 1)) if use_limits else None, upper=np.tile(hi, (B, 1)) if use_limits else None,
                tol=tol, settle_vel=sv, settle_min_dwell=settle_min_dwell, max_dwell=max_dwell,
                fail_reset_after=fail_reset_after, mu_regoal=0.0, counts=True)
    return state, args


# ---------------------------------------------------------------------------------------------------------
# The scripted sequence: 40 calls on one handle, exit flags, speeds and positions per step from the tables below
# ---------------------------------------------------------------------------------------------------------
SEQ_STEPS, SEQ_B, SEQ_POOL = 40, 65, 3
SEQ_PARAMS = dict(settle_min_dwell=2, max_dwell=5, fail_reset_after=3)
# per instance, shifted by b: a run of exactly two failures followed by a success, later a run of exactly three
SEQ_FLAGS = (1, -6, -7, 2, 0, -6, -6, -7, 1, 1, 1, 2, 1)


def sequence_case(name, desc, lim, oracle):
    """(state, args, script): the first call's state (its xinit is script step 0) and per step t the exit flags
    ``script["exitflag"][t]`` and states ``script["xinit"][t]`` the host writes before call t.  The pool's goals lie
    half a tolerance from the end link at known configurations; a scripted state is either one of those (near) or a
    configuration far from all of them, moving or at rest."""
    B, P, T = SEQ_B, SEQ_POOL, SEQ_STEPS
    n, nx, N = desc["n"], desc["nx"], desc["N"]
    nvar = nx + desc["ns"] + desc["nu"]
    tol, sv = TOL[name], SETTLE_VEL[name]
    lo, hi = np.asarray(lim[0], dtype=np.float64), np.asarray(lim[1], dtype=np.float64)
    qp = _inside((lo, hi), B * P, 1).reshape(B, P, n)          # where goal i of instance b is reached
    qfar = _inside((lo, hi), B, 6)
    x_start = np.zeros((B, nx))
    x_start[:, :n] = _inside((lo, hi), B, 4)
    pool = np.zeros((B, P, 3))
    for b in range(B):
        _speeds(desc, x_start[b], 2.0, sv, b)
        for i in range(P):
            x = np.zeros(nx); x[:n] = qp[b, i]
            pool[b, i] = end_link(oracle, desc, x) + 0.5 * tol * DIRS[(b + i) % 7]
    L = len(SEQ_FLAGS)
    exitflag = np.array([[SEQ_FLAGS[(t + b) % L] for b in range(B)] for t in range(T)], dtype=np.int32)
    xs = np.zeros((T, B, nx))
    for t in range(T):
        for b in range(B):
            near = (t + 2 * b) % 7 == 0
            xs[t, b, :n] = qp[b, (t // 7 + b) % P] if near else qfar[b]
            rest = (t + 3 * b) % 11 in (0, 1)
            _speeds(desc, xs[t, b], 0.5 if rest else 2.0, sv, b + t)
    x0 = 1000.0 + np.arange(B * N * nvar, dtype=np.float64).reshape(B, N, nvar) / 8.0
    state = dict(xinit=xs[0].copy(), x0=x0, goal=pool[:, 0].copy(), cursor=np.zeros(B, dtype=np.int32),
                 dwell=np.zeros(B, dtype=np.int32), failrun=np.zeros(B, dtype=np.int32), exitflag=exitflag[0],
                 iters=np.full(B, 3, dtype=np.int32))
    args = dict(oracle=oracle, desc=desc, pool=pool, x_start=x_start, lower=np.tile(lo, (B, 1)), upper=np.tile(hi, (B, 1)),
                tol=tol, settle_vel=sv, mu_regoal=0.0, counts=True, **SEQ_PARAMS)
    return state, args, dict(exitflag=exitflag, xinit=xs)


def flag_script(B):
    """exit flags for the advance: negative at lanes 0, 15, 16 and B - 1 (where they exist) and at every seventh lane
    from 5 on, the other lanes cycle through 1, 2, 0"""
    ef = np.array([(1, 2, 0)[b % 3] for b in range(B)], dtype=np.int32)
    for b in [0, 15, 16, B - 1] + list(range(5, B, 7)):
        if 0 <= b < B:
            ef[b] = -6 if b % 2 == 0 else -7
    return ef


def obstacle_case(B, nobst, dt, arena):
    """od (B, nobst, 9).  Per axis (the same table for x, y and z, each axis at its own place in it): well inside, within
    one step of +arena moving out, within one step of +arena moving in, the same at -arena, and each of them with an
    acceleration.  The walls are those of ``arena`` = 9 whichever arena the call is given."""
    wall = 9.0
    v = 0.5
    step = v * dt
    tab = [(0.3, v, 0.0), (-4.0, -v, 0.2), (wall - 0.5 * step, v, 0.0), (wall - 0.5 * step, -v, 0.0),
           (-wall + 0.5 * step, -v, 0.0), (-wall + 0.5 * step, v, 0.0), (wall - 0.25 * step, v, 0.4),
           (-wall + 0.25 * step, -v, -0.4), (wall - 0.5 * step, 0.5 * v, -0.3), (2.5, 0.0, 1.0), (-wall + 0.1, v, 0.3)]
    od = np.zeros((B, nobst, 9))
    for b in range(B):
        for o in range(nobst):
            i = b * nobst + o
            for c in range(3):
                p, vel, acc = tab[(i + 4 * c + i // 11) % 11]
                # (no two entries alike: a write at another obstacle's place shows)
                od[b, o, c], od[b, o, 3 + c], od[b, o, 6 + c] = p - (1e-3 * (i % 7) + 1e-6 * i) * np.sign(p), vel * (1 + 0.01 * (i % 5)), acc
    return od
