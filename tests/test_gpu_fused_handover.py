"""Instance hand-over of the fused kernels: a half-wavefront of k_fused (a wavefront of k_fused_arm, the cfg4 and chain5
cases) that has finished an instance stores its plan (epilogue), takes the next position of the launch's queue and
copies that instance's rows into its block (prologue).
The arithmetic of an instance must depend neither on its position in the queue, nor on its partner half, nor on how
many hand-overs its half-wavefront has behind it: a launch on a tiny grid (``RMPC_FUSED_GRID``, read at rmpc_create:
every half-wavefront takes many instances, first and later sweeps mix inside a wavefront) returns bit for bit what the
default grid returns, where every instance has a half-wavefront of its own and nothing is handed over.

Fused configurations and the sizes the hand-over copies (npar parameter words and m = rows of multipliers per stage,
N stages; the copies run in sets of 40 words / 36 rows, 16-byte requests from the first 16-byte boundary of a row):

    cfg1 / pointRobot  npar 30  m 31  N 10 / 20      cfg2            npar 38  m 33  N 30
    wc_point           npar 34  m 32  N 12           chain2          npar 33  m 23  N 24   (odd npar)
    cfg3               npar 44  m 36  N 30           boxer           npar 27  m 31  N 10   (odd npar)
    wc_boxer           npar 36  m 36  N 10           wc_boxer_slack  npar 37  m 37  N 12   (odd npar, two sets of rows)

chain2 and wc_boxer_slack have an odd npar: every other stage row of the caller's parameter array starts between two
16-byte boundaries and takes the path with a single word in front.  Both are cases below, and cfg2 with an odd horizon
(time_horizon = 7) has odd b N + k at even npar.

The comparisons with the oracle use the bars of tests/test_gpu_parity.py (check_plan of tests/gpu_support.py)."""
import numpy as np
import pytest

from gpu_support import check_plan

pytestmark = pytest.mark.gpu

KEYS = ("z", "exitflag", "iters", "kkt", "obj")


@pytest.fixture(scope="module")
def rt():
    import __graft_entry__ as g
    g.build()
    from oracle.oracle import Oracle
    from robot_mpcs_amd._lib import Solver
    from robot_mpcs_amd.scenarios import make_scenario
    return dict(Oracle=Oracle, Solver=Solver, make_scenario=make_scenario, check_plan=check_plan)


def _on_grid(rt, sc, B, grid, monkeypatch, run):
    """run(solver) with the fused launch on `grid` wavefronts (None: the default grid, one per SIMD of the chip)"""
    if grid is None:
        monkeypatch.delenv("RMPC_FUSED_GRID", raising=False)
    else:
        monkeypatch.setenv("RMPC_FUSED_GRID", str(grid))   # (read once, at rmpc_create)
    s = rt["Solver"](sc.desc, max_batch=B)
    assert s.is_fused()
    try:
        return run(s)
    finally:
        s.close()


def _solve(sc):
    def run(s):
        r = s.solve(sc.xinit, sc.x0, sc.params)
        return dict(r, last_passes=s.last_passes())
    return run


def _assert_equal(a, b):
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), (key, np.flatnonzero((a[key] != b[key]).reshape(len(a[key]), -1).any(axis=1)))
    assert a["last_passes"] == b["last_passes"], (a["last_passes"], b["last_passes"])


CASES = [
    # name, B, seed, scenario arguments, grid
    ("cfg2", 72, 11, {}, 2),                       # four half-wavefronts, 18 hand-overs each
    ("wc_point", 40, 12, {}, 2),                   # velocity-limit rows, npar 34, m 32
    ("cfg3", 40, 13, {}, 2),                       # the boxer: records through the workspace, runtime tables; npar 44 (two sets)
    ("cfg2", 24, 14, {"time_horizon": 7}, 2),      # lanes >= N idle in the hand-over, odd b N + k
    ("chain2", 40, 15, {}, 2),                     # npar = 33 (odd), m = 23
    ("wc_boxer_slack", 24, 16, {}, 2),             # npar = 37 (odd), m = 37 (two sets of rows), slack variable
    # k_fused_arm: a wavefront per instance, its own epilogue and prologue (copies by stage and half of the wavefront)
    ("cfg4", 12, 17, {}, 2),                       # the panda, N = 20: three parts per stage
    ("cfg4", 10, 19, {"time_horizon": 22}, 2),     # two parts per stage
    ("chain5", 10, 20, {}, 2),                     # five joints
]


@pytest.mark.parametrize("name,B,seed,kw,grid", CASES)
def test_queue_position_changes_nothing(rt, name, B, seed, kw, grid, monkeypatch):
    sc = rt["make_scenario"](name, B=B, seed=seed, **kw)
    tiny = _on_grid(rt, sc, B, grid, monkeypatch, _solve(sc))
    full = _on_grid(rt, sc, B, None, monkeypatch, _solve(sc))
    _assert_equal(tiny, full)
    cpu = rt["Oracle"](sc.desc).solve_batch(sc.xinit, sc.x0, sc.params)
    rt["check_plan"](tiny, cpu, sc.desc["nx"] + sc.desc["ns"])


@pytest.mark.parametrize("B", [1, 3])
def test_halves_without_work(rt, B, monkeypatch):
    """B = 1: the second half of the only wavefront never gets an instance.  B = 3 on one wavefront: the queue is empty
    when the first half to finish asks, it retires while its partner continues."""
    sc = rt["make_scenario"]("cfg2", B=B, seed=21)
    one = _on_grid(rt, sc, B, 1, monkeypatch, _solve(sc))
    full = _on_grid(rt, sc, B, None, monkeypatch, _solve(sc))
    _assert_equal(one, full)
    cpu = rt["Oracle"](sc.desc).solve_batch(sc.xinit, sc.x0, sc.params)
    rt["check_plan"](one, cpu, sc.desc["nx"] + sc.desc["ns"])


@pytest.mark.parametrize("name,B,seed", [("cfg2", 72, 31), ("cfg3", 40, 32), ("cfg4", 12, 33)])
def test_warm_path_through_the_epilogue(rt, name, B, seed, monkeypatch):
    """Warm-start mode: the epilogue leaves the multipliers, mu and the pass counts; the second solve starts from them,
    its queue ordered longest first."""
    sc = rt["make_scenario"](name, B=B, seed=seed)

    def run(s):
        s.set_warm_start(True)
        first = s.solve(sc.xinit, sc.x0, sc.params)
        first = dict(first, last_passes=s.last_passes())
        second = s.solve(sc.xinit, first["z"].copy(), sc.params)
        return first, dict(second, last_passes=s.last_passes())

    t1, t2 = _on_grid(rt, sc, B, 2, monkeypatch, run)
    f1, f2 = _on_grid(rt, sc, B, None, monkeypatch, run)
    _assert_equal(t1, f1)
    _assert_equal(t2, f2)
    assert t2["iters"].sum() < t1["iters"].sum(), (t1["iters"].sum(), t2["iters"].sum())   # the multipliers did arrive


def test_mode_switch(rt, monkeypatch):
    """A cold handle keeps no multipliers: switched to warm-start mode its next solve is the cold first solve of a
    warm-mode handle, and switched back it solves cold again."""
    B = 72
    sc = rt["make_scenario"]("cfg2", B=B, seed=41)

    def switched(s):
        cold = s.solve(sc.xinit, sc.x0, sc.params)
        s.set_warm_start(True)
        a = s.solve(sc.xinit, sc.x0, sc.params)
        w = s.solve(sc.xinit, a["z"].copy(), sc.params)      # warm: from the multipliers `a` left
        s.set_warm_start(False)
        c = s.solve(sc.xinit, sc.x0, sc.params)
        return cold, a, w, c

    def fresh_warm(s):
        s.set_warm_start(True)
        a = s.solve(sc.xinit, sc.x0, sc.params)
        return a, s.solve(sc.xinit, a["z"].copy(), sc.params)

    for grid in (2, None):
        cold, a, w, c = _on_grid(rt, sc, B, grid, monkeypatch, switched)
        fa, fw = _on_grid(rt, sc, B, grid, monkeypatch, fresh_warm)
        for key in KEYS:
            assert np.array_equal(a[key], fa[key]), (grid, key)
            assert np.array_equal(w[key], fw[key]), (grid, key)
            assert np.array_equal(c[key], cold[key]), (grid, key)
        assert w["iters"].sum() < a["iters"].sum()


def test_deadline(rt, monkeypatch):
    """set_pass_budget(6): instances cut while active leave through the epilogue with flag 0.  No cold cfg2 instance
    finishes within 6 passes (oracle: at least 11 on every instance of the seeds 0 .. 39), so the budget cuts a whole
    cold batch; the mix of cut and finished instances is the warm second solve of seed 0 (oracle, orc_solve_warm from
    the first solve's plan and multipliers: 50 of the 72 instances need at most 6 passes, 22 need 7 .. 13)."""
    B = 72
    sc = rt["make_scenario"]("cfg2", B=B, seed=0)

    def run(s):
        s.set_pass_budget(6)
        cold = dict(s.solve(sc.xinit, sc.x0, sc.params), last_passes=s.last_passes())
        s.set_pass_budget(0)
        s.set_warm_start(True)
        free = s.solve(sc.xinit, sc.x0, sc.params)
        s.set_pass_budget(6)
        cut = dict(s.solve(sc.xinit, free["z"].copy(), sc.params), last_passes=s.last_passes())
        return cold, cut

    tc, tw = _on_grid(rt, sc, B, 2, monkeypatch, run)
    fc, fw = _on_grid(rt, sc, B, None, monkeypatch, run)
    _assert_equal(tc, fc)
    _assert_equal(tw, fw)
    assert np.all(tc["exitflag"] == 0) and np.all(tc["iters"] < 6) and np.all(np.isfinite(tc["z"]))
    was_cut = tw["exitflag"] == 0
    print("warm solve under a budget of 6 passes: %d cut, %d finished" % (was_cut.sum(), (~was_cut).sum()))
    assert was_cut.sum() > 0 and (~was_cut).sum() > 0, (was_cut.sum(), (~was_cut).sum())
    assert np.all(tw["exitflag"][~was_cut] >= 1) and np.all(np.isfinite(tw["z"]))
    assert tw["last_passes"] == 6
