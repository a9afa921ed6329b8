"""The kernels that carry the steady closed loop from one control step to the next -- ``rmpc_retarget_device``
(k_retarget), ``rmpc_advance_device_flags`` (k_advance) and ``rmpc_advance_obstacles_device`` (k_obst_advance) --
against the numpy restatements of tests/steady_loop_reference.py on the constructed inputs of
tests/steady_loop_cases.py (which tests/test_steady_loop_cpu.py pins and inspects on the CPU).  The integer state
machine is compared bit for bit; the only floating-point decisions in it (distance against tol, speed against
settle_vel, joints against the widened box) are kept at least 2 % from their thresholds by construction, which every
test asserts on the restatement's margins."""
import ctypes as C

import numpy as np
import pytest

import steady_loop_cases as cases
from gpu_support import DEV
from steady_loop_reference import advance_step, obstacles_step, retarget_step

pytestmark = pytest.mark.gpu

MAX_B = 300
STATE_KEYS = ("xinit", "x0", "goal", "cursor", "dwell", "failrun")


@pytest.fixture(scope="module")
def rt():
    import torch
    import __graft_entry__ as g
    g.build()
    from oracle.oracle import Oracle
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.scenarios import LIMITS, make_scenario
    robots, solvers = {}, {}

    def robot(name):
        """descriptor, joint-limit box, oracle and a solver handle (one per config for the whole module)"""
        if name not in robots:
            desc = make_scenario(name, B=1, seed=0).desc
            solvers[name] = _lib.Solver(desc, max_batch=MAX_B)
            robots[name] = (desc, LIMITS[name][0], Oracle(desc), solvers[name])
        return robots[name]

    yield dict(torch=torch, Oracle=Oracle, lib=_lib, Solver=_lib.Solver, make_scenario=make_scenario, limits=LIMITS, robot=robot)
    for s in solvers.values():
        s.close()


def _margins(r):
    return min(r["margin_dist"].min(), r["margin_vel"].min(), r["margin_joint"].min())


class Device:
    """The arrays of one retarget call on the device.  The pool sits in front of NaNs, the counters start from distinct
    values and their reserved entries from zero."""
    COUNT_BASE = 100 * (np.arange(16, dtype=np.int64) + 1) * (np.arange(16) < 13)

    def __init__(self, rt, state, args, counts=True, pool_pad=64):
        torch = rt["torch"]
        self.torch = torch
        f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)
        i32 = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)
        B, P = args["pool"].shape[:2]
        self.B = B
        padded = np.full((B * P + pool_pad, 3), np.nan)
        padded[:B * P] = args["pool"].reshape(B * P, 3)
        self.pool_store = f64(padded)
        self.pool = self.pool_store[:B * P].view(B, P, 3)
        self.t = dict(xinit=f64(state["xinit"]), x0=f64(state["x0"]), goal=f64(state["goal"]), cursor=i32(state["cursor"]),
                      dwell=i32(state["dwell"]), failrun=i32(state.get("failrun")), exitflag=i32(state.get("exitflag")),
                      iters=i32(state.get("iters")), x_start=f64(args["x_start"]),
                      lower=None if args.get("lower") is None else f64(args["lower"]),
                      upper=None if args.get("upper") is None else f64(args["upper"]),
                      counts=torch.from_numpy(self.COUNT_BASE.copy()).to(DEV) if counts else None)

    def write(self, **arrays):
        for k, a in arrays.items():
            dt = np.int32 if self.t[k].dtype == self.torch.int32 else np.float64
            self.t[k].copy_(self.torch.from_numpy(np.ascontiguousarray(a, dtype=dt)))

    def call(self, s, args):
        t = self.t
        s.retarget_device(self.B, t["xinit"], t["x0"], t["exitflag"], t["goal"], self.pool, t["cursor"], t["dwell"],
                          t["x_start"], args["tol"], args["max_dwell"], counts=t["counts"], iters=t["iters"],
                          mu_regoal=args.get("mu_regoal", 0.0), failrun=t["failrun"],
                          fail_reset_after=args["fail_reset_after"], settle_vel=args["settle_vel"],
                          settle_min_dwell=args["settle_min_dwell"], lower_limits=t["lower"], upper_limits=t["upper"])
        self.torch.cuda.synchronize()

    def read(self):
        out = {k: (None if self.t[k] is None else self.t[k].cpu().numpy()) for k in STATE_KEYS}
        out["counts"] = None if self.t["counts"] is None else self.t["counts"].cpu().numpy() - self.COUNT_BASE
        return out


def _same_state(got, ref, where=""):
    for k in STATE_KEYS:
        if ref[k] is None:
            assert got[k] is None
            continue
        bad = np.flatnonzero((got[k] != ref[k]).reshape(got[k].shape[0], -1).any(axis=1))
        assert bad.size == 0, (where, k, bad[:8], ref["event"][bad[0]])


def _same_counts(got, want):
    """bit-equal but [9], the sum of floor(dist 1e6): one unit per hand-over for the last ulp of the distance"""
    print("counts", got.tolist(), "reference", want)
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12):
        assert got[k] == want[k], (k, int(got[k]), want[k])
    assert abs(int(got[9]) - want[9]) <= want[10], (int(got[9]), want[9], want[10])
    assert np.all(got[13:16] == 0)


def _untouched(got, state, ref):
    quiet = np.array([e == "none" for e in ref["event"]])
    for k in ("xinit", "x0", "goal"):
        assert np.array_equal(got[k][quiet], state[k][quiet]), k


# ---------------------------------------------------------------------------------------------------------
# a. one call on constructed instances
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg2", "cfg3", "cfg4"])
@pytest.mark.parametrize("B,P", [(1, 3), (63, 1), (64, 3), (65, 1), (257, 3), (300, 3)])
def test_retarget_single_step(rt, name, B, P):
    desc, lim, o, s = rt["robot"](name)
    state, args = cases.retarget_case(name, desc, lim, o, B, P)
    ref = retarget_step(state, args)
    assert _margins(ref) >= 1e-6
    d = Device(rt, state, args)
    d.call(s, args)
    got = d.read()
    _same_state(got, ref)
    _same_counts(got["counts"], ref["counts"])
    _untouched(got, state, ref)


# ---------------------------------------------------------------------------------------------------------
# b. the optional arrays
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", ["counts", "iters", "failrun", "limits", "exitflag"])
def test_retarget_optional_pointers(rt, missing):
    desc, lim, o, s = rt["robot"]("cfg4")
    opt = dict(failrun=dict(use_failrun=False, fail_reset_after=1), limits=dict(use_limits=False),
               exitflag=dict(use_flags=False)).get(missing, {})
    state, args = cases.retarget_case("cfg4", desc, lim, o, 65, 3, **opt)
    if missing == "iters":
        state["iters"] = None
    args["counts"] = missing != "counts"
    ref = retarget_step(state, args)
    assert _margins(ref) >= 1e-6
    if missing in ("failrun", "limits"):
        assert "reset" in ref["event"]      # by the first failure / by the fail run alone
    d = Device(rt, state, args, counts=args["counts"])
    d.call(s, args)
    got = d.read()
    _same_state(got, ref)
    if args["counts"]:
        _same_counts(got["counts"], ref["counts"])
        if missing == "exitflag":
            assert np.all(got["counts"][4:9] == 0) and got["counts"][11] == 0
        if missing == "iters":
            assert got["counts"][8] == 0 and got["counts"][4:8].sum() == 65
    _untouched(got, state, ref)


# ---------------------------------------------------------------------------------------------------------
# c. forty calls on one handle
# ---------------------------------------------------------------------------------------------------------
def test_retarget_scripted_sequence(rt):
    desc, lim, o, s = rt["robot"]("cfg2")
    state, args, script = cases.sequence_case("cfg2", desc, lim, o)
    d = Device(rt, state, args)
    total = [0] * 13
    for t in range(cases.SEQ_STEPS):
        state = dict(state, xinit=script["xinit"][t], exitflag=script["exitflag"][t])
        d.write(xinit=state["xinit"], exitflag=state["exitflag"])
        ref = retarget_step(state, args)
        assert _margins(ref) >= 1e-6, t
        d.call(s, args)
        _same_state(d.read(), ref, where=t)
        total = [a + b for a, b in zip(total, ref["counts"])]
        state = dict(state, **{k: ref[k] for k in STATE_KEYS})
    assert np.all(state["cursor"] >= 2 * cases.SEQ_POOL) and total[0] and total[1] and total[2] and total[3]
    _same_counts(d.read()["counts"], total)      # incremented call after call, not overwritten


# ---------------------------------------------------------------------------------------------------------
# d. the barrier restart after a hand-over
# ---------------------------------------------------------------------------------------------------------
def _two_solves(rt, sc, mu_regoal, scripted, dwell, pool):
    """solve, plant step, retarget with scripted flags, solve: what the second solve returned, and the state the
    retarget call saw"""
    torch = rt["torch"]
    from robot_mpcs_amd.fleet import dev_f64, limit_tensors, make_block, step_block
    B = sc.B
    f = make_block(sc.desc, sc.setup["mpc"]["weights"], B, sc.xinit, DEV, x0=sc.x0, goal=dev_f64(pool[:, 0], DEV),
                   r_body=dev_f64(np.full(B, sc.extra["r_body"]), DEV), obst_dyn=dev_f64(sc.extra["obst_dyn"], DEV),
                   **limit_tensors(*rt["limits"]["cfg3"], B, DEV))
    s = f["s"]
    s.set_warm_start(True)
    step_block(f, previous_plan=True)
    torch.cuda.synchronize()
    first = dict(ef=f["ef"].cpu().numpy().copy(), x=f["x"].cpu().numpy().copy())
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)
    cursor, dw, flags, tpool, start = i32(np.zeros(B)), i32(dwell), i32(scripted), dev_f64(pool, DEV), dev_f64(sc.xinit, DEV)
    s.retarget_device(B, f["x"], f["x0"], flags, f["goal"], tpool, cursor, dw, start, tol=1e-9, max_dwell=2,
                      mu_regoal=mu_regoal)
    step_block(f, previous_plan=True)
    torch.cuda.synchronize()
    out = dict(z=f["z"].cpu().numpy().copy(), ef=f["ef"].cpu().numpy().copy(), it=f["it"].cpu().numpy().copy(),
               goal=f["goal"].cpu().numpy().copy(), cursor=cursor.cpu().numpy(), first=first, fused=s.is_fused())
    s.close()
    return out


@pytest.mark.parametrize("fused", [True, False])
def test_barrier_restart_reaches_its_own_instance_only(rt, fused, monkeypatch):
    if fused:
        monkeypatch.delenv("RMPC_NO_FUSED", raising=False)
    else:
        monkeypatch.setenv("RMPC_NO_FUSED", "1")    # (read once, at rmpc_create): the pass kernels hold their own array
    B = 64
    sc = rt["make_scenario"]("cfg3", B=B, seed=41)
    scripted = np.array([cases.FLAGS[b % 5] for b in range(B)], dtype=np.int32)
    # (every third instance keeps its goal, the first one among them: a restart written to the head of the array instead
    #  of the instance's own place lands on an instance that must not change)
    dwell = np.array([1 if b % 3 != 0 else 0 for b in range(B)], dtype=np.int32)   # second step on the goal: timed out
    pool = np.stack([sc.extra["goal"], sc.extra["goal"] + np.array([1.0, -1.0, 0.0])], axis=1)
    a = _two_solves(rt, sc, 0.0, scripted, dwell, pool)
    b = _two_solves(rt, sc, 0.1, scripted, dwell, pool)
    assert a["fused"] == fused and b["fused"] == fused
    assert np.array_equal(a["first"]["x"], b["first"]["x"]) and np.array_equal(a["first"]["ef"], b["first"]["ef"])
    assert np.all(a["first"]["ef"] >= 0)       # every instance has multipliers and a barrier parameter to warm-start from
    # the restatement says who took a new goal and whose restart was requested
    desc = sc.desc
    state = dict(xinit=a["first"]["x"], x0=np.zeros((B, desc["N"], desc["nx"] + desc["ns"] + desc["nu"])), goal=pool[:, 0],
                 cursor=np.zeros(B, dtype=np.int32), dwell=dwell, failrun=None, exitflag=scripted, iters=None)
    ref = retarget_step(state, dict(oracle=rt["Oracle"](desc), desc=desc, pool=pool, x_start=sc.xinit, lower=None, upper=None,
                                    tol=1e-9, settle_vel=0.0, settle_min_dwell=0, max_dwell=2, fail_reset_after=0,
                                    mu_regoal=0.1))
    took = np.array([e != "none" for e in ref["event"]])
    assert np.array_equal(took, dwell == 1) and set(ref["event"]) == {"none", "late"}
    for r in (a, b):
        assert np.array_equal(r["cursor"], ref["cursor"]) and np.array_equal(r["goal"], ref["goal"])
    restart = np.zeros(B, dtype=bool)
    restart[sorted(ref["regoal"])] = True
    assert np.array_equal(restart, took & (scripted >= 0))
    kept, took_failed = ~took, took & (scripted < 0)
    assert kept[0] and not restart[0]
    assert kept.sum() >= 10 and took_failed.sum() >= 10 and restart.sum() >= 10
    same = np.array([np.array_equal(a["z"][i], b["z"][i]) and a["ef"][i] == b["ef"][i] and a["it"][i] == b["it"][i]
                     for i in range(B)])
    print("instances that differ:", np.flatnonzero(~same).tolist(), "restart requested:", np.flatnonzero(restart).tolist())
    assert np.all(same[kept]), np.flatnonzero(kept & ~same)
    assert np.all(same[took_failed]), np.flatnonzero(took_failed & ~same)
    assert np.any(~same[restart])


# ---------------------------------------------------------------------------------------------------------
# e. the plant step and the next initial guess, with exit flags
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plans(rt):
    """one real solve of 40 instances per config, made when first asked for"""
    made = {}

    def get(name):
        if name not in made:
            sc = rt["make_scenario"](name, B=40, seed=31)
            s = rt["robot"](name)[3]
            made[name] = (sc, s.solve(sc.xinit, sc.x0, sc.params))
        return made[name]

    return get


@pytest.mark.parametrize("prev", [True, False])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 40])
@pytest.mark.parametrize("name", ["cfg2", "cfg3", "cfg4"])
def test_advance_with_flags(rt, plans, name, B, prev):
    torch = rt["torch"]
    sc40, r = plans(name)
    desc, _, o, s = rt["robot"](name)
    xinit, z = sc40.xinit[:B].copy(), r["z"][:B].copy()
    ef = cases.flag_script(B)
    assert ef[0] < 0 and ef[B - 1] < 0 and (B < 17 or (ef[15] < 0 and ef[16] < 0 and 0 < (ef[1:15] >= 0).sum() < 14))
    tz, tx, te = torch.from_numpy(z).to(DEV), torch.from_numpy(xinit).to(DEV), torch.from_numpy(ef).to(DEV)
    t0 = torch.full((B, desc["N"], s.nvar), float("nan"), dtype=torch.float64, device=DEV)
    s.advance_device(B, tz, tx, t0, previous_plan=prev, exitflag=te)
    torch.cuda.synchronize()
    xn_dev, got = tx.cpu().numpy(), t0.cpu().numpy()
    pk = rt["make_scenario"](name, B=B, seed=31).packer
    xn, x0_ref = advance_step(o, pk, xinit, z, ef, prev)
    np.testing.assert_allclose(xn_dev, xn, rtol=0, atol=1e-14)
    assert not np.isnan(got).any()
    # an instance that shifts its plan copies numbers of the plan only: bit for bit
    shifts = (ef >= 0) & prev
    assert np.array_equal(got[shifts], x0_ref[shifts]), np.flatnonzero(shifts)
    # an instance that restarts repeats its new state, which the line above allows to differ from the oracle's in the
    # last place: bit for bit the restatement's guess from the state the device has written
    want = advance_step(o, pk, xinit, z, ef, prev, x_new=xn_dev)[1]
    bad = np.flatnonzero((got != want).reshape(B, -1).any(axis=1))
    assert bad.size == 0, (bad, ef[bad])
    print("restarting instances bit-equal to the oracle-fed guess too:", bool(np.array_equal(got, x0_ref)))
    assert np.array_equal(tz.cpu().numpy(), z) and np.array_equal(te.cpu().numpy(), ef)


# ---------------------------------------------------------------------------------------------------------
# f. the moving obstacles
# ---------------------------------------------------------------------------------------------------------
EPS = 2.0 ** -53


def _obstacles(rt, od, dt, arena):
    torch = rt["torch"]
    t = torch.from_numpy(od.copy()).to(DEV)
    L = rt["lib"].load_library()
    rc = L.rmpc_advance_obstacles_device(od.shape[0], od.shape[1], float(dt), float(arena), C.c_void_p(t.data_ptr()), None)
    assert rc == 0, L.rmpc_last_error()
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("arena", [0.0, 9.0])
@pytest.mark.parametrize("B,nobst", [(1, 1), (3, 5), (64, 4), (257, 3)])
def test_obstacles_step_and_reflection(rt, B, nobst, arena):
    dt = rt["robot"]("cfg3")[0]["dt"]
    od = cases.obstacle_case(B, nobst, dt, arena)
    # one step: |pos - ref| <= 4 eps (S_pos + 2 arena), |vel - ref| <= 2 eps S_vel (three-term sum, products possibly
    # contracted, then the mirroring 2 arena - pos); ten steps: the same sums, step after step along the reference
    got, cur, bound_p, bound_v = od, od, 0.0, 0.0
    for step in range(10):
        ref, s_pos, s_vel, raw = obstacles_step(cur, dt, arena)
        if arena > 0:
            assert np.abs(np.abs(raw) - arena).min() >= 1e-6 * arena      # the branch is decided alike
            if step == 0 and B * nobst >= 11:
                assert (np.abs(raw[:, :, :2]) > arena).sum() >= 3 and (np.abs(raw[:, :, 2]) > arena).sum() >= 3
        got = _obstacles(rt, got, dt, arena)
        if step == 0:
            one_p, one_v = 4 * EPS * (s_pos + 2 * arena), 2 * EPS * s_vel
            ep, ev = np.abs(got[:, :, 0:3] - ref[:, :, 0:3]), np.abs(got[:, :, 3:6] - ref[:, :, 3:6])
            print("one step: max err / bound, pos %.3f vel %.3f" % (float((ep / one_p).max()), float((ev / np.maximum(one_v, 1e-300)).max())))
            assert np.all(ep <= one_p) and np.all(ev <= one_v)
            if arena == 0:
                assert np.array_equal(np.sign(got[:, :, 3:6]), np.sign((od[:, :, 3:6] + od[:, :, 6:9] * dt)))
        assert np.array_equal(got[:, :, 6:9], od[:, :, 6:9])
        bound_p = np.maximum(bound_p, 4 * EPS * (s_pos + 2 * arena))
        bound_v = np.maximum(bound_v, 2 * EPS * s_vel)
        cur = ref
    ep, ev = np.abs(got[:, :, 0:3] - ref[:, :, 0:3]), np.abs(got[:, :, 3:6] - ref[:, :, 3:6])
    print("ten steps: max err / (10 x bound), pos %.3f vel %.3f" % (float((ep / (10 * bound_p)).max()),
                                                                   float((ev / np.maximum(10 * bound_v, 1e-300)).max())))
    assert np.all(ep <= 10 * bound_p) and np.all(ev <= 10 * bound_v)


# ---------------------------------------------------------------------------------------------------------
# g. what the host refuses, without a launch
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["struct_size", "pool_len", "x_start", "batch"])
def test_retarget_refusals(rt, what):
    torch = rt["torch"]
    lib = rt["lib"]
    desc, lim, o, _ = rt["robot"]("cfg2")
    B = 5
    s = rt["Solver"](desc, max_batch=4 if what == "batch" else B)
    state, args = cases.retarget_case("cfg2", desc, lim, o, B, 3)
    d = Device(rt, state, args)
    t = d.t
    p = lambda x: x.data_ptr()
    a = lib.RetargetArgs()
    a.struct_size = C.sizeof(lib.RetargetArgs) + (1 if what == "struct_size" else 0)
    a.pool_len = 0 if what == "pool_len" else 3
    a.xinit, a.x0, a.exitflag, a.iters, a.goal = p(t["xinit"]), p(t["x0"]), p(t["exitflag"]), p(t["iters"]), p(t["goal"])
    a.goal_pool, a.x_start = p(d.pool), (None if what == "x_start" else p(t["x_start"]))
    a.cursor, a.dwell, a.failrun = p(t["cursor"]), p(t["dwell"]), p(t["failrun"])
    a.lower_limits, a.upper_limits = p(t["lower"]), p(t["upper"])
    a.tol, a.settle_vel, a.mu_regoal = args["tol"], args["settle_vel"], 0.0
    a.settle_min_dwell, a.max_dwell, a.fail_reset_after, a.reserved = 4, 9, 3, 0
    a.counts = p(t["counts"])
    rc = s._L.rmpc_retarget_device(s._h, B, C.byref(a), None)
    torch.cuda.synchronize()
    assert rc != 0 and s._L.rmpc_last_error()
    got = d.read()
    for k in STATE_KEYS:
        assert np.array_equal(got[k], state[k]), k
    assert np.all(got["counts"] == 0)
    s.close()


@pytest.mark.parametrize("what", ["B", "nobst", "pointer"])
def test_obstacle_refusals(rt, what):
    torch = rt["torch"]
    L = rt["lib"].load_library()
    od = cases.obstacle_case(3, 2, 0.1, 9.0)
    t = torch.from_numpy(od.copy()).to(DEV)
    rc = L.rmpc_advance_obstacles_device(0 if what == "B" else 3, 0 if what == "nobst" else 2, 0.1, 9.0,
                                         None if what == "pointer" else C.c_void_p(t.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc != 0 and L.rmpc_last_error()
    assert np.array_equal(t.cpu().numpy(), od)
