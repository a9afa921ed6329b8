"""A plain restatement of the scene packer: ``rmpc_scene`` -> all_parameters [B][N][npar].

Written from the text of include/rmpc.h (``rmpc_scene``) and the reference planner's loops
(robotmpcs/planner/mpcPlanner.py:83-210: reset, setGoalReaching, setRadialConstraints, setLinearConstraints,
setJointLimits, setVelLimits, setInputLimits, setConstraintAvoidance, updateDynamicObstacles) -- not from
``ParamPacker`` and not from ``k_scene``.  One scalar assignment per word, Python loops over b, k and j, every product
and sum of the obstacle prediction written out in the header's order.  The host packer, the reference-style loops of
reference_style_pack below and the three device layouts are all held to this array (test_scene_cpu.py,
test_gpu_scene_layouts.py)."""
import numpy as np

# the pointer members of rmpc_scene, in the header's order
SCENE_FIELDS = ("goal", "r_body", "obst", "obst_dyn", "lower_limits", "upper_limits", "lower_limits_u", "upper_limits_u",
                "lower_limits_vel", "upper_limits_vel", "lin_constrs")

EMPTY_OBSTACLE = -100.0     # position and radius of the reference's EmptyObstacle (mpcPlanner.py:18-26)


def _flat(a, B, per_instance):
    """host array of one field as B rows of ``per_instance`` words, or None"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(B, per_instance)
    return a


def scene_batch(fields):
    """B of a scene: the leading axis of its first given field"""
    for name in SCENE_FIELDS:
        if fields.get(name) is not None:
            return int(np.shape(fields[name])[0])
    raise ValueError("a scene with no field has no batch size")


def pack_scene_ref(desc, N, weights, dyn_radius, fields):
    """params [B][N][npar] (float64) of the scene ``fields`` (rmpc_scene member name -> host array or None).

    A None field stays zero, with one exception: when both ``obst`` and ``obst_dyn`` are None every obstacle word is
    -100.0.  When both are given ``obst_dyn`` wins; its radius slot is ``dyn_radius``."""
    unknown = set(fields) - set(SCENE_FIELDS)
    if unknown:
        raise KeyError("not members of rmpc_scene: %s" % sorted(unknown))
    B = scene_batch(fields)
    N = int(N)
    n, nu, ns, nobst, npar = int(desc["n"]), int(desc["nu"]), int(desc["ns"]), int(desc["nobst"]), int(desc["npar"])
    n_modules = int(desc["n_modules"]) if "n_modules" in desc else len(desc["module_kind"])
    dt = float(desc["dt"])
    offsets = {key[4:]: int(v) for key, v in desc.items() if key.startswith("off_")}
    off = offsets.__getitem__
    goal = _flat(fields.get("goal"), B, 3)
    r_body = _flat(fields.get("r_body"), B, 1)
    obst = _flat(fields.get("obst"), B, nobst * 4)
    obst_dyn = _flat(fields.get("obst_dyn"), B, nobst * 9)
    lower, upper = _flat(fields.get("lower_limits"), B, n), _flat(fields.get("upper_limits"), B, n)
    lower_u, upper_u = _flat(fields.get("lower_limits_u"), B, nu), _flat(fields.get("upper_limits_u"), B, nu)
    lower_vel, upper_vel = _flat(fields.get("lower_limits_vel"), B, 2), _flat(fields.get("upper_limits_vel"), B, 2)
    lin = _flat(fields.get("lin_constrs"), B, N * nobst * 4)
    w, wu, ws = float(weights.get("w", 0.0)), float(weights.get("wu", 0.0)), float(weights.get("ws", 0.0))
    wconstr = [float(v) for v in weights.get("wconstr", [])]
    dyn_radius = float(dyn_radius)

    out = np.zeros((B, N, npar), dtype=np.float64)
    for b in range(B):
        for k in range(N):
            p = out[b, k]
            # reset(): zeros, then the broadcast weights (:91-104)
            if desc["has_goal"]:
                for j in range(3):
                    p[off("wgoal") + j] = w
            for j in range(nu):
                p[off("wu") + j] = wu
            if ns:
                p[off("ws")] = ws
            # setConstraintAvoidance (:206-210)
            if desc["has_avoid"]:
                for j in range(n_modules):
                    p[off("wconstr") + j] = wconstr[j] if j < len(wconstr) else 0.0
            # setGoalReaching (:197-204)
            if desc["has_goal"] and goal is not None:
                for j in range(3):
                    p[off("goal") + j] = goal[b, j]
            if off("r_body") >= 0 and r_body is not None:
                p[off("r_body")] = r_body[b, 0]
            if off("obst") >= 0:
                if obst_dyn is not None:
                    # updateDynamicObstacles (:144-161): stage k predicted at dt * k
                    kk = float(k)
                    for j in range(nobst):
                        for c in range(3):
                            pos, vel, acc = float(obst_dyn[b, 9 * j + c]), float(obst_dyn[b, 9 * j + 3 + c]), float(obst_dyn[b, 9 * j + 6 + c])
                            tk = dt * kk
                            lin_term = (vel * dt) * kk
                            quad_term = (0.5 * (tk * tk)) * acc
                            p[off("obst") + 4 * j + c] = (pos + lin_term) + quad_term
                        p[off("obst") + 4 * j + 3] = dyn_radius
                elif obst is not None:
                    # setRadialConstraints (:120-133)
                    for j in range(4 * nobst):
                        p[off("obst") + j] = obst[b, j]
                else:
                    for j in range(4 * nobst):
                        p[off("obst") + j] = EMPTY_OBSTACLE
            # setLinearConstraints (:135-141): plane j of stage k
            if off("lin") >= 0 and lin is not None:
                for j in range(4 * nobst):
                    p[off("lin") + j] = lin[b, k * 4 * nobst + j]
            # setJointLimits (:167-175), setInputLimits (:187-195), setVelLimits (:177-185)
            if off("lower") >= 0 and lower is not None:
                for j in range(n):
                    p[off("lower") + j] = lower[b, j]
            if off("upper") >= 0 and upper is not None:
                for j in range(n):
                    p[off("upper") + j] = upper[b, j]
            if off("lower_u") >= 0 and lower_u is not None:
                for j in range(nu):
                    p[off("lower_u") + j] = lower_u[b, j]
            if off("upper_u") >= 0 and upper_u is not None:
                for j in range(nu):
                    p[off("upper_u") + j] = upper_u[b, j]
            if off("lower_vel") >= 0 and lower_vel is not None:
                for j in range(2):
                    p[off("lower_vel") + j] = lower_vel[b, j]
            if off("upper_vel") >= 0 and upper_vel is not None:
                for j in range(2):
                    p[off("upper_vel") + j] = upper_vel[b, j]
    return out


def reference_style_pack(pm, npar, N, cfg, calls):
    """One instance's flat parameter vector by per-element loops exactly as the reference planner writes them, its
    expression for the predicted obstacles included (``calls``: the setters in the order they are called)."""
    p = np.zeros(npar * N)
    for i in range(N):
        if "wgoal" in pm:
            p[[npar * i + v for v in pm["wgoal"]]] = cfg.weights["w"]
        p[[npar * i + v for v in pm["wu"]]] = cfg.weights["wu"]
        if cfg.slack:
            p[[npar * i + v for v in pm["ws"]]] = cfg.weights["ws"]
    for name, args in calls:
        for i in range(N):
            if name == "radial":
                pos, rad, r_body = args
                p[npar * i + pm["r_body"][0]] = r_body
                for j in range(cfg.number_obstacles):
                    pj, rj = (pos[j], rad[j]) if j < len(pos) else ([-100, -100, -100], -100)
                    for m_i in range(3):
                        p[npar * i + pm["obst"][j * 4 + m_i]] = pj[m_i]
                    p[npar * i + pm["obst"][j * 4 + 3]] = rj
            elif name == "joint":
                for j in range(cfg.n):
                    p[npar * i + pm["lower_limits"][j]] = args[0][j]
                    p[npar * i + pm["upper_limits"][j]] = args[1][j]
            elif name == "input":
                for j in range(len(pm["lower_limits_u"])):
                    p[npar * i + pm["lower_limits_u"][j]] = args[0][j]
                    p[npar * i + pm["upper_limits_u"][j]] = args[1][j]
            elif name == "goal":
                for j in range(3):
                    p[npar * i + pm["goal"][j]] = args[j] if j < len(args) else 0
            elif name == "avoid":
                p[[npar * i + v for v in pm["wconstr"]]] = cfg.weights["wconstr"]
            elif name == "dyn":
                obst, dt, r = args
                nb = obst.size // 9
                for j in range(cfg.number_obstacles):
                    if j < nb:
                        pos, vel, acc = obst[9 * j: 9 * j + 3], obst[9 * j + 3: 9 * j + 6], obst[9 * j + 6: 9 * j + 9]
                    else:
                        pos, vel, acc = np.ones(3) * -100, np.zeros(3), np.zeros(3)
                    for m_i in range(3):
                        p[npar * i + pm["obst"][j * 4 + m_i]] = pos[m_i] + vel[m_i] * dt * i + 0.5 * (dt * i) ** 2 * acc[m_i]
                    p[npar * i + pm["obst"][j * 4 + 3]] = r
    return p
