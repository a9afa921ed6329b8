"""The merged sweep call of the point robot's fused kernel (generated view, records in LDS): on a pass that starts a
fresh step the call requests the stage's words once, forms the step lengths from them and continues into the sweep
from registers.  Passes that are NOT fresh -- the null pass after a failed curvature step, a line-search retry, the
first pass, a pass cut by the budget -- must behave as before, also when the two halves of a wavefront differ.  They
are rare for this robot, so the batches below are chosen by what the oracle does on them
(``Oracle.solve`` + ``orc_last_passes()``; a solve without such a pass needs iterations + 1 passes):

  cfg2, B = 191, seed 7                    5 instances with more passes than iterations + 1 (null passes; the slowest
                                           needs 28 iterations in 32 passes); odd batch: one half idles at the end
  cfg2, B = 191, seed 1                    2 such instances
  cfg2, B = 63, seed 3, time_horizon = 12  1 such instance and one accepted step with a line-search retry; 20 of the
                                           32 lanes of a half have no stage
  cfg1, B = 9, seed 7                      the example model's view (one distance row), odd batch

The default path (view, merged call) is compared with the runtime-table path (RMPC_NO_SPEC=1: the step lengths come
from a separate step call) at the bars of tests/test_spec_gen.py, and with the oracle: equal flags on every instance,
iteration counts at the bar of tests/test_gpu_parity.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import __graft_entry__ as g
    g.build()
    from oracle.oracle import Oracle, lib as olib
    from robot_mpcs_amd._lib import Solver
    from robot_mpcs_amd.scenarios import make_scenario
    return dict(Oracle=Oracle, olib=olib, Solver=Solver, make_scenario=make_scenario)


def _both_paths(rt, sc, B, monkeypatch, run):
    """run(solver) on the view and on the runtime tables"""
    out = []
    for no_spec in (False, True):
        if no_spec:
            monkeypatch.setenv("RMPC_NO_SPEC", "1")     # (read once, at rmpc_create)
        else:
            monkeypatch.delenv("RMPC_NO_SPEC", raising=False)
        s = rt["Solver"](sc.desc, max_batch=B)
        assert (s.spec_name() == "") == no_spec
        out.append(run(s))
        s.close()
    return out


def _same_as_tables(ra, rb):
    # tests/test_spec_gen.py: same arithmetic, differently contracted multiply-adds
    assert np.mean(ra["exitflag"] == rb["exitflag"]) >= 0.99
    same = (ra["exitflag"] == rb["exitflag"]) & (ra["iters"] == rb["iters"]) & np.isin(ra["exitflag"], (1, 2))
    assert same.mean() >= 0.97, same.mean()
    scale = np.maximum(1.0, np.abs(rb["z"]).max(axis=(1, 2)))
    err = np.abs(ra["z"] - rb["z"]).max(axis=(1, 2)) / scale
    print("view vs tables: equal flags %.4f, same %.4f, max plan error %.3e" % (np.mean(ra["exitflag"] == rb["exitflag"]), same.mean(), err[same].max()))
    assert err[same].max() <= 1e-8, err[same].max()


def _oracle_passes(rt, sc, B):
    o = rt["Oracle"](sc.desc)
    flag, iters, passes = np.zeros(B, dtype=int), np.zeros(B, dtype=int), np.zeros(B, dtype=int)
    for b in range(B):
        r = o.solve(sc.xinit[b], sc.x0[b], sc.params[b])
        flag[b], iters[b], passes[b] = r["exitflag"], r["iters"], rt["olib"]().orc_last_passes()
    return flag, iters, passes


CASES = [
    # name, B, seed, scenario arguments, instances with passes > iterations + 1 (oracle)
    ("cfg2", 191, 7, {}, 5),
    ("cfg2", 191, 1, {}, 2),
    ("cfg2", 63, 3, {"time_horizon": 12}, 1),
    ("cfg1", 9, 7, {}, None),
]


@pytest.mark.parametrize("name,B,seed,kw,extra", CASES)
def test_merged_call_equals_step_call_and_oracle(rt, name, B, seed, kw, extra, monkeypatch):
    sc = rt["make_scenario"](name, B=B, seed=seed, **kw)
    flag, iters, passes = _oracle_passes(rt, sc, B)
    if extra is not None:
        # the batch does contain passes that are not fresh
        assert int((passes > iters + 1).sum()) == extra, (passes - iters - 1)
    ra, rb = _both_paths(rt, sc, B, monkeypatch, lambda s: s.solve(sc.xinit, sc.x0, sc.params))
    _same_as_tables(ra, rb)
    print("view vs oracle: flags differ on %d, iterations equal %.4f" % ((ra["exitflag"] != flag).sum(), (ra["iters"] == iters).mean()))
    assert np.array_equal(ra["exitflag"], flag), np.flatnonzero(ra["exitflag"] != flag)
    assert (ra["iters"] == iters).mean() >= 0.98


def test_merged_call_warm_start(rt, monkeypatch):
    """Second solve of a handle with the multipliers of the first: its first pass reads the previous solve's
    multipliers one stage on (no step lengths), the passes after it the current buffer."""
    B = 191
    sc = rt["make_scenario"]("cfg2", B=B, seed=7)

    def run(s):
        s.set_warm_start(True)
        first = s.solve(sc.xinit, sc.x0, sc.params)
        x0w = first["z"].copy()
        return first, s.solve(sc.xinit, x0w, sc.params)

    (a1, a2), (b1, b2) = _both_paths(rt, sc, B, monkeypatch, run)
    _same_as_tables(a1, b1)
    _same_as_tables(a2, b2)
    assert a2["iters"].mean() < a1["iters"].mean()   # (the warm start did start warm)


@pytest.mark.parametrize("budget", [14, 29])
def test_merged_call_under_a_pass_budget(rt, budget, monkeypatch):
    """A budget cuts solves in the middle: 14 passes most of the slow ones, 29 those with null passes (the slowest
    instance of this batch needs 32).  What finishes is what finishes without a budget; both paths cut the same."""
    B = 191
    sc = rt["make_scenario"]("cfg2", B=B, seed=7)

    def run(s):
        free = s.solve(sc.xinit, sc.x0, sc.params)
        s.set_pass_budget(budget)
        cut = s.solve(sc.xinit, sc.x0, sc.params)
        s.set_pass_budget(0)
        return free, cut

    (fa, ca), (fb, cb) = _both_paths(rt, sc, B, monkeypatch, run)
    done = ca["exitflag"] != 0
    assert 0 < done.sum() < B, done.sum()
    assert np.array_equal(ca["exitflag"][done], fa["exitflag"][done]) and np.array_equal(ca["iters"][done], fa["iters"][done])
    assert np.array_equal(ca["z"][done], fa["z"][done])
    assert np.all(np.isfinite(ca["z"][~done])) and np.all(ca["iters"][~done] < budget)
    assert np.mean((ca["exitflag"] != 0) == (cb["exitflag"] != 0)) >= 0.99
    _same_as_tables(fa, fb)
    both = done & (cb["exitflag"] != 0)
    _same_as_tables({k: ca[k][both] for k in ("z", "exitflag", "iters")}, {k: cb[k][both] for k in ("z", "exitflag", "iters")})
