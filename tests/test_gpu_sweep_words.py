"""The merged sweep call of the point robot's fused kernel (generated view, chain without slack) moves fewer words per
pass and asks for the step lengths' operands first (SWEEPWORDS, rmpc_sweep.hpp): the values of the twelve general
single-variable rows are neither stored nor read back but formed from the stored iterate and the limit -- by the
expression that formed the stored word, so every bit is the parent's -- and the order of the requests changes no
operation.  Every batch of tests/sweep_words_cases.py (which says what each one exercises and how its seed was chosen) is

  * at the oracle's flags and iteration counts, instance by instance, with the most passes of the launch
    (last_passes()) equal to the oracle's -- that is the regime the case was chosen for,
  * within check_plan's tolerance of the oracle's plan,
  * at the flags and iteration counts of the runtime tables (RMPC_NO_SPEC=1, read when the handle is created), whose
    sweep stores the rows' values and whose step lengths read them back as before,
  * byte for byte the five result arrays that the commit before this change returned for the same inputs
    (tests/golden/sweep_words_parent.npz, recorded with that commit's library on an MI355X by
    tests/golden/make_sweep_words_parent.py).
"""
import contextlib
import os

import numpy as np
import pytest

import sweep_words_cases as cs
from gpu_support import check_plan

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_words_parent.npz")
SWITCHES = ("RMPC_NO_SPEC", "RMPC_FUSED_GRID")


@contextlib.contextmanager
def _switches(**env):
    """the switches a handle reads when it is created, set for the block and put back after it"""
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


@pytest.fixture(scope="module")
def rt():
    import __graft_entry__ as g
    g.build()
    from oracle.oracle import Oracle, lib as olib
    from robot_mpcs_amd._lib import Solver
    from robot_mpcs_amd.scenarios import make_scenario
    scs = {key: cs.scenario(make_scenario, key) for key in cs.BATCHES}
    return dict(Oracle=Oracle, olib=olib, Solver=Solver, sc=scs)


def _oracle_batch(rt, sc, x0, params):
    """the oracle's plans of a batch (solve_batch) and its passes per instance"""
    o = rt["Oracle"](sc.desc)
    r = dict(o.solve_batch(sc.xinit, x0, params))
    passes = np.zeros(sc.B, dtype=int)
    for b in range(sc.B):
        one = o.solve(sc.xinit[b], x0[b], params[b])
        assert (one["exitflag"], one["iters"]) == (r["exitflag"][b], r["iters"][b])
        passes[b] = rt["olib"]().orc_last_passes()
    r["passes"] = passes
    return r


@pytest.fixture(scope="module")
def oracle(rt):
    """per batch: the oracle's plans and passes; b3 also warm and damaged"""
    out = {key: _oracle_batch(rt, sc, sc.x0, sc.params) for key, sc in rt["sc"].items()}
    sc = rt["sc"]["b3"]
    cold, warm = cs.oracle_warm_pair(rt["Oracle"], rt["olib"], sc)
    assert np.array_equal(cold["z"], out["b3"]["z"]) and np.array_equal(cold["passes"], out["b3"]["passes"])
    out["warm"] = warm
    x0, P = cs.bad_inputs(sc)
    out["bad"] = _oracle_batch(rt, sc, x0, P)
    return out


@pytest.fixture(scope="module")
def view(rt, oracle):
    with _switches():
        return cs.solve_all(rt["Solver"], rt["sc"].__getitem__, oracle["b3"]["z"])


@pytest.fixture(scope="module")
def tables(rt, oracle):
    with _switches(RMPC_NO_SPEC="1"):
        s = rt["Solver"](rt["sc"]["b3"].desc, max_batch=3)
        assert s.spec_name() == ""
        s.close()
        return cs.solve_all(rt["Solver"], rt["sc"].__getitem__, oracle["b3"]["z"])


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _report(what, gpu, cpu):
    print("%s: flags gpu %s oracle %s, iterations gpu %s oracle %s, passes gpu %d oracle %s" % (
        what, gpu["exitflag"].tolist(), cpu["exitflag"].tolist(), gpu["iters"].tolist(), cpu["iters"].tolist(),
        gpu["last_passes"], cpu["passes"].tolist()))


def _equals_oracle(gpu, cpu, sc):
    assert np.array_equal(gpu["exitflag"], cpu["exitflag"]) and np.array_equal(gpu["iters"], cpu["iters"])
    assert gpu["last_passes"] == cpu["passes"].max()
    check_plan(gpu, cpu, sc.desc["nx"] + sc.desc["ns"])


def _equals_tables(a, b):
    assert np.array_equal(a["exitflag"], b["exitflag"]) and np.array_equal(a["iters"], b["iters"])
    assert a["last_passes"] == b["last_passes"]


def _equals_parent(key, gpu, golden):
    for k in cs.KEYS:
        assert cs.same_bytes(gpu[k], golden["%s_%s" % (key, k)]), (key, k)


@pytest.mark.parametrize("key", sorted(cs.BATCHES))
def test_batch(rt, oracle, view, tables, golden, key):
    sc, cpu, gpu = rt["sc"][key], oracle[key], view[key]
    _report(key, gpu, cpu)
    want = cs.BATCHES[key][4]
    if want is not None:
        assert tuple(cpu["passes"]) == want      # (the regime the seed was chosen for)
    assert np.isin(cpu["exitflag"], (1, 2)).all()   # (every plan is compared)
    if key in ("b3", "lim"):
        # one instance with passes that are not fresh steps: its current buffer holds the row values of an older sweep
        assert (cpu["passes"] > cpu["iters"] + 1).sum() == 1
    if key in ("n2", "n3"):
        assert sc.desc["N"] == int(key[1])
    if key == "lim":
        # every limit word differs from stage to stage and from instance to instance, and thrust limits are active
        d = sc.desc
        P = np.asarray(sc.params).reshape(sc.B, d["N"], d["npar"])
        L = P[:, :, cs.LIM_WORDS[0]:cs.LIM_WORDS[1]].reshape(-1, cs.LIM_WORDS[1] - cs.LIM_WORDS[0])
        assert all(len(np.unique(L[:, w])) == len(L) for w in range(L.shape[1]))
        u = cpu["z"][:, :, d["nx"]:d["nx"] + 3]
        act = (np.abs(u - P[:, :, 19:22]) < 1e-3) | (np.abs(u - P[:, :, 22:25]) < 1e-3)
        assert act.any(axis=(1, 2)).all()
    _equals_oracle(gpu, cpu, sc)
    _equals_tables(gpu, tables[key])
    _equals_parent(key, gpu, golden)


def test_half_changes_instance_beside_an_iterating_partner(rt, oracle, view, golden):
    """b3 on one wavefront (RMPC_FUSED_GRID=1): the half of instance 0 hands over to instance 2 while its partner
    iterates, so both copies of the call -- the first-pass one, which no longer stores the general rows' values, and
    the later-pass one, which no longer reads them -- run in one pass.  The arrays of the default grid, and the parent's
    on one wavefront."""
    sc, cpu = rt["sc"]["b3"], oracle["b3"]
    p = cpu["passes"]
    assert p[0] < p[1] < p[0] + p[2]   # half 0 is first, takes instance 2 and ends last
    with _switches(RMPC_FUSED_GRID="1"):
        s = rt["Solver"](sc.desc, max_batch=3)
        gpu = dict(s.solve(sc.xinit, sc.x0, sc.params), last_passes=s.last_passes())
        s.close()
    _report("b3 on one wavefront", gpu, cpu)
    _equals_oracle(gpu, cpu, sc)
    for k in cs.KEYS:
        assert cs.same_bytes(gpu[k], view["b3"][k]), k
    _equals_parent("b3g1", gpu, golden)


def test_warm_started_solve_on_the_same_handle(rt, oracle, view, tables, golden):
    sc, cpu, gpu = rt["sc"]["b3"], oracle["warm"], view["warm"]
    _report("warm", gpu, cpu)
    assert np.isin(cpu["exitflag"], (1, 2)).all()
    assert cpu["iters"].sum() < oracle["b3"]["iters"].sum() / 2   # (it did start warm)
    _equals_oracle(gpu, cpu, sc)
    _equals_tables(gpu, tables["warm"])
    _equals_parent("warm", gpu, golden)


def test_first_pass_meets_a_bad_row_value(rt, oracle, view, tables, golden):
    """The damaged batch of the row-sums cases: a non-positive value under the inverse-barrier term (instance 1) and a
    non-finite row value (instance 2) end the solve on its first pass with the oracle's flag; instance 0, the partner
    half of instance 1, converges as in the undamaged batch."""
    sc, cpu, gpu = rt["sc"]["b3"], oracle["bad"], view["bad"]
    _report("bad", gpu, cpu)
    assert tuple(cpu["exitflag"]) == cs.BAD_FLAGS and tuple(cpu["passes"][1:]) == (1, 1)
    assert np.array_equal(gpu["exitflag"], cpu["exitflag"]) and np.array_equal(gpu["iters"], cpu["iters"])
    assert gpu["last_passes"] == cpu["passes"].max()
    assert np.array_equal(gpu["z"][0], view["b3"]["z"][0])
    check_plan(gpu, cpu, sc.desc["nx"] + sc.desc["ns"])
    _equals_tables(gpu, tables["bad"])
    _equals_parent("bad", gpu, golden)
