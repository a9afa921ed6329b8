"""Early hand-over of k_fused: a half-wavefront whose instance stops at the decision of a pass stores its plan, takes the
next instance of the queue and runs that instance's first sweep and first decision at once (round 1 of the pass), so
that its first recursion shares the call with the partner's.  The deadline (``set_pass_budget``) stays
at the top of the pass, a pass has at most two rounds, and what an instance computes depends neither on the site at
which its half took it nor on its partner.

Every case runs on a tiny grid (``RMPC_FUSED_GRID``, read at rmpc_create: a wavefront takes instance after instance,
so nearly every instance is taken at an early hand-over) and on the default grid (every instance has a half-wavefront
of its own: nothing is handed over), compares the two bit for bit, and checks the tiny grid's result against the oracle
at the bars of tests/test_gpu_parity.py (``check_plan``).  The fused configurations and their sizes are listed in
tests/test_gpu_fused_handover.py.

An instance that stops at its FIRST decision: searched with the oracle (``solve_each``, passes per instance) in cfg1,
cfg2, wc_point, cfg3, chain2, boxer, wc_boxer and wc_boxer_slack, seeds 0 .. 3 with B = 24, cold, warm from the own plan
and multipliers, and warm once more: no shipped scenario has one (cold at least 9 passes, warm at least 4).  The case
below damages instances of a cfg2 batch instead -- their initial guess lies inside the first obstacle on every stage
behind the pinned one, a non-positive row under the inverse-barrier term: flag -7 at the first decision, as in
tests/sweep_row_sums_cases.py."""
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
    return dict(Oracle=Oracle, Solver=Solver, make_scenario=make_scenario)


def _on_grid(rt, desc, B, grid, monkeypatch, run):
    """run(solver) with the fused launch on `grid` wavefronts (None: the default grid, one per SIMD of the chip)"""
    if grid is None:
        monkeypatch.delenv("RMPC_FUSED_GRID", raising=False)
    else:
        monkeypatch.setenv("RMPC_FUSED_GRID", str(grid))   # (read once, at rmpc_create)
    s = rt["Solver"](desc, max_batch=B)
    assert s.is_fused()
    try:
        return run(s)
    finally:
        s.close()


def _solve(xinit, x0, params):
    def run(s):
        return dict(s.solve(xinit, x0, params), last_passes=s.last_passes())
    return run


def _assert_equal(a, b):
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), (key, np.flatnonzero((a[key] != b[key]).reshape(len(a[key]), -1).any(axis=1)))
    assert a["last_passes"] == b["last_passes"], (a["last_passes"], b["last_passes"])


def _tiny_against_default_and_oracle(rt, sc, B, grid, monkeypatch, x0=None, params=None):
    x0 = sc.x0 if x0 is None else x0
    params = sc.params if params is None else params
    tiny = _on_grid(rt, sc.desc, B, grid, monkeypatch, _solve(sc.xinit, x0, params))
    full = _on_grid(rt, sc.desc, B, None, monkeypatch, _solve(sc.xinit, x0, params))
    _assert_equal(tiny, full)
    cpu = rt["Oracle"](sc.desc).solve_batch(sc.xinit, x0, params)
    check_plan(tiny, cpu, sc.desc["nx"] + sc.desc["ns"])
    return tiny, cpu


CASES = [
    # name, B, seed, scenario arguments, grid
    # the queue runs dry at an early hand-over: the last instance is taken there (B = 3), a half retires there while its
    # partner continues, the last two stop and find the queue empty
    ("cfg2", 3, 51, {}, 1),
    ("cfg2", 4, 52, {}, 1),
    ("cfg2", 5, 53, {}, 1),
    ("cfg2", 6, 54, {}, 1),
    ("cfg2", 9, 55, {}, 2),                        # two wavefronts share a queue of five
    # runtime tables, records through the workspace, a step phase behind the shared recursion
    ("cfg3", 24, 56, {}, 1),
    ("cfg3", 24, 56, {}, 2),
    ("wc_boxer_slack", 16, 57, {}, 1),
    ("wc_boxer_slack", 16, 57, {}, 2),
    ("chain2", 24, 58, {}, 2),                     # the n = 2 recursion, npar = 33 (odd)
    ("cfg2", 16, 59, {"time_horizon": 7}, 1),      # the lanes >= N idle through a round-1 sweep
]


@pytest.mark.parametrize("name,B,seed,kw,grid", CASES)
def test_early_hand_over_changes_nothing(rt, name, B, seed, kw, grid, monkeypatch):
    sc = rt["make_scenario"](name, B=B, seed=seed, **kw)
    _tiny_against_default_and_oracle(rt, sc, B, grid, monkeypatch)


@pytest.mark.parametrize("budget", [1, 2])
def test_budget_cuts_at_the_top_of_the_pass(rt, budget, monkeypatch):
    """A cold cfg2 instance needs at least 11 passes (oracle): under a budget of 1 or 2 passes every instance is cut at
    the top of a pass, behind its recursion, and none leaves through the early hand-over.  Flag 0 and `budget` passes."""
    B = 24
    sc = rt["make_scenario"]("cfg2", B=B, seed=0)

    def run(s):
        s.set_pass_budget(budget)
        return dict(s.solve(sc.xinit, sc.x0, sc.params), last_passes=s.last_passes())

    tiny = _on_grid(rt, sc.desc, B, 1, monkeypatch, run)
    full = _on_grid(rt, sc.desc, B, None, monkeypatch, run)
    _assert_equal(tiny, full)
    assert np.all(tiny["exitflag"] == 0) and np.all(np.isfinite(tiny["z"]))
    assert np.all(tiny["iters"] < budget)
    assert tiny["last_passes"] == budget


def test_budget_and_early_hand_over_in_one_wavefront(rt, monkeypatch):
    """The warm second solve under a budget of 6 passes, as test_deadline of tests/test_gpu_fused_handover.py, on one
    wavefront: instances that finish within the budget leave behind their decision, the others at the top of a pass.
    Oracle, cfg2 seed 0 with B = 24, warm from the first solve's plan and multipliers: 20 instances need at most 6
    passes (4 .. 6), 4 need 7 or 8."""
    B = 24
    sc = rt["make_scenario"]("cfg2", B=B, seed=0)

    def run(s):
        s.set_warm_start(True)
        free = dict(s.solve(sc.xinit, sc.x0, sc.params), last_passes=s.last_passes())
        s.set_pass_budget(6)
        cut = dict(s.solve(sc.xinit, free["z"].copy(), sc.params), last_passes=s.last_passes())
        return free, cut

    tf, tw = _on_grid(rt, sc.desc, B, 1, monkeypatch, run)
    ff, fw = _on_grid(rt, sc.desc, B, None, monkeypatch, run)
    _assert_equal(tf, ff)
    _assert_equal(tw, fw)
    cpu = rt["Oracle"](sc.desc).solve_batch(sc.xinit, sc.x0, sc.params)
    check_plan(tf, cpu, sc.desc["nx"] + sc.desc["ns"])
    was_cut = tw["exitflag"] == 0
    print("warm solve under a budget of 6 passes: %d cut, %d finished" % (was_cut.sum(), (~was_cut).sum()))
    assert was_cut.sum() > 0 and (~was_cut).sum() > 0, (was_cut.sum(), (~was_cut).sum())
    assert np.all(tw["exitflag"][~was_cut] >= 1) and np.all(np.isfinite(tw["z"]))
    assert tw["last_passes"] == 6


def test_partner_changes_nothing(rt, monkeypatch):
    """Queue in index order (RMPC_NO_COLD_ORDER, read at rmpc_create) on one wavefront: the batch and its reverse pair
    every instance with other partners and hand it over at other sites and passes; its result is the same bytes."""
    B = 24
    sc = rt["make_scenario"]("cfg2", B=B, seed=61)
    monkeypatch.setenv("RMPC_NO_COLD_ORDER", "1")
    fwd, cpu = _tiny_against_default_and_oracle(rt, sc, B, 1, monkeypatch)
    rev = _on_grid(rt, sc.desc, B, 1, monkeypatch,
                   _solve(sc.xinit[::-1].copy(), sc.x0[::-1].copy(), sc.params[::-1].copy()))
    _assert_equal(fwd, dict({key: rev[key][::-1] for key in KEYS}, last_passes=rev["last_passes"]))


def test_stop_at_the_first_decision(rt, monkeypatch):
    """Instances 2, 3, 4 and 6 of 8 start inside their first obstacle: flag -7 at their first decision.  In index order on
    one wavefront the half that finishes first takes instance 2 at an early hand-over: it stops inside round 1 and waits
    for the top of the next pass (at most two rounds); instance 3 is taken there, stops in round 0, and instance 4 is
    taken behind it in round 1 of the same pass."""
    B = 8
    sc = rt["make_scenario"]("cfg2", B=B, seed=62)
    d = sc.desc
    N, npar = d["N"], d["npar"]
    P = np.array(sc.params, dtype=np.float64).reshape(B, N, npar)
    x0 = np.array(sc.x0, dtype=np.float64).copy()
    damaged = [2, 3, 4, 6]
    for b in damaged:
        c = P[b, 1, d["off_obst"]:d["off_obst"] + 2]
        x0[b, 1:, 0] = c[0]
        x0[b, 1:, 1] = c[1] + 0.05
    monkeypatch.setenv("RMPC_NO_COLD_ORDER", "1")
    tiny, cpu = _tiny_against_default_and_oracle(rt, sc, B, 1, monkeypatch, x0=x0)
    assert cpu["exitflag"][damaged].tolist() == [-7] * len(damaged), cpu["exitflag"]
    assert tiny["exitflag"][damaged].tolist() == [-7] * len(damaged) and np.all(tiny["iters"][damaged] == 0)
    ok = np.setdiff1d(np.arange(B), damaged)
    assert np.all(tiny["exitflag"][ok] >= 1), tiny["exitflag"]
