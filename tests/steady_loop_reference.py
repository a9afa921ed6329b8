"""Plain numpy restatements of the three device entries that carry the steady closed loop from one control step to
the next, written from the text of include/rmpc.h: ``rmpc_retarget_device`` (``retarget_step``),
``rmpc_advance_device_flags`` (``advance_step``) and ``rmpc_advance_obstacles_device`` (``obstacles_step``).
Sequential, one instance after the other, exact integers; nothing here looks at the kernels' arrays or order of
evaluation.  tests/test_steady_loop_cpu.py pins them on hand-worked cases, tests/test_gpu_steady_loop.py compares the
kernels with them."""
import numpy as np

ROBOT_DIFFDRIVE = 1   # RMPC_ROBOT_DIFFDRIVE
N_COUNTS = 13         # counts[0..12] are written, [13..15] are reserved
EVENTS = ("none", "arrived", "settled", "late", "reset")


def end_link(oracle, desc, x):
    """Position of the descriptor's end frame at the configuration x[0..n)."""
    return oracle.fk(np.asarray(x, dtype=np.float64)[:desc["n"]], desc["end_frame"])[0]


def speed(desc, x):
    """Largest joint speed of a chain (nx = 2n), largest of x[6], x[7] of the diff-drive base."""
    if desc["robot"] == ROBOT_DIFFDRIVE:
        return max(abs(float(x[6])), abs(float(x[7])))
    n = desc["n"]
    return max(abs(float(v)) for v in x[n:2 * n])


def retarget_step(state, args):
    """One call of ``rmpc_retarget_device`` for all B instances.

    ``state``: xinit (B, nx), x0 (B, N, nvar), goal (B, 3), cursor (B,), dwell (B,), failrun (B,) or None, exitflag (B,)
    or None, iters (B,) or None.  ``args``: oracle, desc, pool (B, P, 3), x_start (B, nx), lower / upper (B, n) or None,
    tol, settle_vel, settle_min_dwell, max_dwell, fail_reset_after, mu_regoal, and counts (bool, default True: a counter
    array is handed in).

    Returns a dict: the new xinit, x0, goal, cursor, dwell, failrun (None when none was given), ``counts`` (the
    increments of counts[0..12], python ints; all zero without a counter array), ``regoal`` (the set of instances whose
    barrier restart was requested), ``event`` (per instance, one of EVENTS), ``dist`` (per instance) and the margins of
    the floating-point decisions: ``margin_dist`` = |dist - tol| / tol, ``margin_vel`` = |vmax - settle_vel| / settle_vel
    (inf when settle_vel = 0), ``margin_joint`` (B, n, 2) = distance of each joint to lo - 0.05 (hi - lo) and to
    hi + 0.05 (hi - lo) relative to hi - lo (inf without limits)."""
    oracle, desc = args["oracle"], args["desc"]
    xinit = np.array(state["xinit"], dtype=np.float64)
    x0 = np.array(state["x0"], dtype=np.float64)
    goal = np.array(state["goal"], dtype=np.float64)
    cursor = np.array(state["cursor"], dtype=np.int64)
    dwell = np.array(state["dwell"], dtype=np.int64)
    failrun = None if state.get("failrun") is None else np.array(state["failrun"], dtype=np.int64)
    exitflag, iters = state.get("exitflag"), state.get("iters")
    pool, x_start = np.asarray(args["pool"], dtype=np.float64), np.asarray(args["x_start"], dtype=np.float64)
    lower, upper = args.get("lower"), args.get("upper")
    tol, settle_vel = float(args["tol"]), float(args["settle_vel"])
    settle_min, max_dwell, reset_after = int(args["settle_min_dwell"]), int(args["max_dwell"]), int(args["fail_reset_after"])
    mu_regoal = float(args.get("mu_regoal", 0.0))
    counting = bool(args.get("counts", True))
    B, nx, n, P = xinit.shape[0], desc["nx"], desc["n"], pool.shape[1]
    counts = [0] * N_COUNTS
    regoal, event = set(), []
    dist_out, m_dist, m_vel = np.zeros(B), np.zeros(B), np.full(B, np.inf)
    m_joint = np.full((B, n, 2), np.inf)

    for b in range(B):
        ef = None if exitflag is None else int(exitflag[b])
        if counting and ef is not None:
            for slot, hit in ((4, ef == 1), (5, ef == 2), (6, ef == 0), (7, ef < 0)):
                counts[slot] += int(hit)
            if iters is not None:
                counts[8] += int(iters[b])
        failed = ef is not None and ef < 0
        # 1. the fail run
        fr = (int(failrun[b]) if failrun is not None else 0) + 1 if failed else 0
        # 2. reset: outside the widened joint-limit box, or the fail run has reached its length
        oob = False
        if lower is not None and upper is not None:
            for j in range(n):
                lo, hi = float(lower[b, j]), float(upper[b, j])
                q = float(xinit[b, j])
                oob = oob or q < lo - 0.05 * (hi - lo) or q > hi + 0.05 * (hi - lo)
                m_joint[b, j, 0] = abs(q - (lo - 0.05 * (hi - lo))) / (hi - lo)
                m_joint[b, j, 1] = abs(q - (hi + 0.05 * (hi - lo))) / (hi - lo)
        reset = oob or (failed and reset_after > 0 and fr >= reset_after)
        if oob:
            counts[12] += 1
        if reset:
            xinit[b] = x_start[b]
            x0[b] = 0.0
            x0[b, :, :nx] = x_start[b]
            fr = 0
        if failrun is not None:
            failrun[b] = fr
        if fr > 0:
            counts[11] += 1
        # 3. the three events on the state after step 2
        d = end_link(oracle, desc, xinit[b]) - goal[b]
        dist = float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
        vmax = speed(desc, xinit[b])
        dist_out[b] = dist
        m_dist[b] = abs(dist - tol) / tol
        if settle_vel > 0.0:
            m_vel[b] = abs(vmax - settle_vel) / settle_vel
        dw = int(dwell[b]) + 1
        arrived = dist < tol
        settled = (not arrived) and settle_vel > 0.0 and dw >= settle_min and vmax < settle_vel
        late = max_dwell > 0 and dw >= max_dwell
        # 4. the hand-over, counted once: reset before arrived before settled before late
        if reset or arrived or settled or late:
            cursor[b] += 1
            goal[b] = pool[b, int(cursor[b]) % P]
            dw = 0
            if mu_regoal > 0.0 and not failed:
                regoal.add(b)
            what = "reset" if reset else "arrived" if arrived else "settled" if settled else "late"
            counts[{"reset": 3, "arrived": 0, "settled": 1, "late": 2}[what]] += 1
            if not reset:
                counts[9] += int(np.floor(dist * 1e6))
                counts[10] += 1
            event.append(what)
        else:
            event.append("none")
        dwell[b] = dw

    if not counting:
        counts = [0] * N_COUNTS
    return dict(xinit=xinit, x0=x0, goal=goal, cursor=cursor, dwell=dwell, failrun=failrun, counts=counts, regoal=regoal,
                event=event, dist=dist_out, margin_dist=m_dist, margin_vel=m_vel, margin_joint=m_joint)


def advance_step(oracle, packer, xinit, z_prev, exitflag, previous_plan, x_new=None):
    """``rmpc_advance_device_flags``: the plant step xinit <- Phi(xinit, first control of z_prev) with the oracle's map,
    and the next solve's initial guess from the packer: ``setX0("previous_plan")`` for the instances with flag >= 0
    (every instance when ``exitflag`` is None) when ``previous_plan`` is set, ``setX0("current_state")`` for the rest.
    Returns (xinit_new (B, nx), x0 (B, N, nvar)).  ``x_new``: build the initial guess from this new state instead of the
    oracle's (a guess that restarts from the state repeats it; a caller that has compared the plant step to its
    tolerance hands the compared state in to compare the repetition bit for bit)."""
    xinit = np.asarray(xinit, dtype=np.float64)
    z_prev = np.asarray(z_prev, dtype=np.float64)
    B = xinit.shape[0]
    nxs = oracle.nx + oracle.ns
    xn = np.stack([oracle.dynamics(xinit[b], z_prev[b, 0, nxs:]) for b in range(B)])
    xg = xn if x_new is None else np.asarray(x_new, dtype=np.float64)

    def guess(kind):
        packer.reset()
        packer._initial_step = False
        return np.array(packer.setX0(xg, z_prev, kind))

    shifted, cold = guess("previous_plan"), guess("current_state")
    shift = np.zeros(B, dtype=bool)
    if previous_plan:
        shift[:] = True if exitflag is None else np.asarray(exitflag) >= 0
    return xn, np.where(shift[:, None, None], shifted, cold)


def obstacles_step(od, dt, arena):
    """``rmpc_advance_obstacles_device`` in ``np.longdouble``: od (..., 9) = position, velocity, acceleration;
    pos += vel dt + acc dt^2 / 2, vel += acc dt; arena > 0: a position beyond +-arena in x or y is mirrored at that wall
    together with its velocity component.  Returns (ref (longdouble, same shape), S_pos (..., 3), S_vel (..., 3), raw
    (..., 3)): the magnitude sums |pos| + |vel dt| + |acc dt^2 / 2| and |vel| + |acc dt| of the inputs, and the
    position before the mirroring (whose distance to the walls says how safely the branch is decided)."""
    o = np.asarray(od).astype(np.longdouble)     # (a longdouble input is kept: several steps in a row without rounding)
    dt, arena = np.longdouble(dt), np.longdouble(arena)
    pos, vel, acc = o[..., 0:3], o[..., 3:6], o[..., 6:9]
    half = np.longdouble(0.5)
    raw = pos + vel * dt + half * acc * dt * dt
    new_vel = vel + acc * dt
    s_pos = (np.abs(pos) + np.abs(vel * dt) + np.abs(half * acc * dt * dt)).astype(np.float64)
    s_vel = (np.abs(vel) + np.abs(acc * dt)).astype(np.float64)
    new_pos = raw.copy()
    if arena > 0:
        for c in (0, 1):
            over, under = raw[..., c] > arena, raw[..., c] < -arena
            new_pos[..., c] = np.where(over, 2 * arena - raw[..., c], np.where(under, -2 * arena - raw[..., c], raw[..., c]))
            new_vel[..., c] = np.where(over | under, -new_vel[..., c], new_vel[..., c])
    ref = np.concatenate([new_pos, new_vel, acc], axis=-1)
    return ref, s_pos, s_vel, raw.astype(np.float64)
