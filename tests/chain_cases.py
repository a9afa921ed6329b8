"""Chains that mix revolute and prismatic joints (tests only): the scenarios of the hand-written assets under
tests/golden/chains/ and the table of their classes.  Used by test_chain_kinematics_cpu.py and
test_gpu_chain_kinematics.py; DESIGN.md 6.3.

The shipped chains are the point robot (P P R, identity origin rotations, coordinate axes) and the panda with its cuts
(all revolute about local z, origin rotations a pure roll).  mix.urdf has the joints R P R R P R R P, every origin
rotation with roll, pitch and yaw, axes off the coordinate axes and not normalised; aff.urdf is P R R.  The classes
run over the runtime tables (no generated view).

`make_chain_scenario(name, B, seed, **mpc_overrides)` has the signature of `scenarios.make_scenario`, so
newton_step_cases.make_inputs and exact_hessian_cases.make_inputs take it unchanged.  Every start pose is strictly
feasible: the sphere stays CLEAR off every collision link, the pairs CLEAR apart, the joints inside their limits.
"""
import os

import numpy as np

import chain_reference as cref

CHAIN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chains")
MODEL = "mixchain"
R_BODY = 0.03
R_OBST = 0.08
CLEAR = 0.06                 # least distance of a row from zero at the start pose
Q_START, Q_GOAL = 0.4, 0.6   # start and goal configurations: uniform in +- these
LIMITS = (-1.0, 1.0)
LIMITS_U = (-5.0, 5.0)

# use_curv, from the rule and not read back from the library: a chain of more than three joints always
# carries the terms (with the kinematics' own second derivatives); one of three or fewer only when every frame of a
# distance row and, with a goal cost, the end frame moves affinely with q -- no revolute joint before the frame's own.
#   mix2  R P      rows on l1 (affine) and l2 (behind the revolute joint 1): off
#   mix3  R P R    rows on l2, l3 and the pair (l1, l3): off
#   aff3  P R R    rows on l1, l2 (affine); the goal on l3, behind the revolute joint 2: off
#   aff3g P R      rows on l1, l2, goal on l2: on
# paths: what a handle of the class runs by default and under the switches (test_gpu_chain_kinematics.py).
CLASSES = {
    "mix2": dict(urdf="mix.urdf", n=2, N=12, use_curv=0, family="small"),
    "mix3": dict(urdf="mix.urdf", n=3, N=10, use_curv=0, family="small"),
    "aff3": dict(urdf="aff.urdf", n=3, N=12, use_curv=0, family="small"),
    "aff3g": dict(urdf="aff.urdf", n=2, N=12, use_curv=1, family="small"),
    "mix5": dict(urdf="mix.urdf", n=5, N=12, use_curv=1, family="arm"),
    "mix7": dict(urdf="mix.urdf", n=7, N=10, use_curv=1, family="arm"),
    "mix4": dict(urdf="mix.urdf", n=4, N=10, use_curv=1, family="pass"),
    "mix8": dict(urdf="mix.urdf", n=8, N=10, use_curv=1, family="pass"),
}
NAMES = tuple(CLASSES)
NO_TERMS = tuple(k for k, v in CLASSES.items() if not v["use_curv"])


def config_file(name):
    return os.path.join(CHAIN_DIR, MODEL, name + "Mpc.yaml")


def urdf_file(name):
    return os.path.join(CHAIN_DIR, MODEL, CLASSES[name]["urdf"])


def reference_chain(name):
    """chain_reference.read_chain of the class: the URDF up to the class's end link l<n>."""
    return cref.read_chain(urdf_file(name), "l%d" % CLASSES[name]["n"])


def make_chain_scenario(name, B=None, seed=0, **mpc_overrides):
    from robot_mpcs_amd.models.mpcModel import normalise_descriptor
    from robot_mpcs_amd.scenarios import Scenario, _packer_for, build_model
    from robot_mpcs_amd.utils.urdf_chain import fk_positions

    if name not in CLASSES:
        raise KeyError(name)
    B = int(B if B is not None else 1)
    model, setup = build_model(config_file(name), asset_dir=CHAIN_DIR, **mpc_overrides)
    desc = normalise_descriptor(model._model)
    pk = _packer_for(model, setup, B)
    rng = np.random.default_rng(seed)
    n = model._n
    links = [int(f) for f in desc["link_frame"]]
    pairs = [(int(a), int(b)) for a, b in desc["pair_frame"]]
    frames = sorted(set(links) | {f for p in pairs for f in p} | {int(desc["end_frame"])})

    q0 = np.zeros((B, n)); opos = np.zeros((B, 1, 3))
    todo = np.ones(B, dtype=bool)
    for _ in range(1000):
        if not todo.any():
            break
        k = int(todo.sum())
        q = rng.uniform(-Q_START, Q_START, size=(k, n))
        fks = fk_positions(desc["joints"], q, frames)
        lp = np.stack([fks[f] for f in links], axis=1)                      # [k, links, 3]
        # the sphere: around a collision link drawn at random, CLEAR .. CLEAR + 0.25 off the nearest link
        pick = lp[np.arange(k), rng.integers(0, len(links), size=k)]
        dirn = rng.normal(size=(k, 3)); dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
        c = pick + dirn * (R_OBST + R_BODY + rng.uniform(CLEAR, CLEAR + 0.25, size=(k, 1)))
        ok = np.all(np.linalg.norm(lp - c[:, None, :], axis=2) - R_OBST - R_BODY >= CLEAR, axis=1)
        for a, b in pairs:
            ok &= np.linalg.norm(fks[a] - fks[b], axis=1) - 2.0 * R_BODY >= CLEAR
        idx = np.flatnonzero(todo)[ok]
        q0[idx] = q[ok]; opos[idx, 0] = c[ok]
        todo[idx] = False
    assert not todo.any(), "no feasible start pose drawn for %s" % name
    qg = rng.uniform(-Q_GOAL, Q_GOAL, size=(B, n))
    goal = fk_positions(desc["joints"], qg, [int(desc["end_frame"])])[int(desc["end_frame"])]

    xinit = np.zeros((B, model._nx))
    xinit[:, :n] = q0
    pk.setRadialConstraints(opos, np.full((B, 1), R_OBST), R_BODY)
    pk.setSelfCollisionAvoidanceConstraints(R_BODY)
    pk.setJointLimits(np.array([[LIMITS[0]] * n, [LIMITS[1]] * n]))
    pk.setInputLimits(np.array([[LIMITS_U[0]] * n, [LIMITS_U[1]] * n]))
    pk.setGoalReaching(goal)
    pk.setConstraintAvoidance()
    x0 = pk.setX0(xinit, None, "current_state").copy()
    return Scenario(name=name, model=model, setup=setup, desc=desc, packer=pk, xinit=xinit, x0=x0,
                    params=pk.params.copy(), extra=dict(goal=goal, r_body=R_BODY, obst_pos=opos, q_goal=qg))
