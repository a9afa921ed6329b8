"""The oracle's branch census (oracle/rmpc_oracle.h ORC_CEN_*) and the witnesses of decision_cases.py, on the CPU:
  * counting changes no result: the census build reproduces the golden vectors bit for bit;
  * the census agrees with what the trace of the same solve shows;
  * every committed witness still takes its branches, finishes within the pass limit and passes the rounding filter
    (flag, iterations, passes and census unchanged under eight relative perturbations of 1e-8 of its inputs) -- a
    later change of the algorithm that un-reaches a branch fails here and names the case;
  * the table branch x model class is complete: every pair has a witness, is excluded by a Cfg flag, or is one of at
    most three pairs listed as unreached.
"""
import json
import os

import numpy as np
import pytest

import decision_cases as dc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# pairs a search had reached before the table was committed (the issue that asked for it): never to be listed as unreached
MUST_HAVE = (
    [("arm", b) for b in ("gn_backtrack", "ls_memory", "curv_halved", "curv_ls_fail", "fact_fail", "latch_set",
                          "latch_released", "restart", "rho_raised", "flag-7")]
    + [("chain3", b) for b in ("cs_retry", "cs_kept", "cs_doubled", "restart", "curv_ls_fail", "back4", "flag2")])


@pytest.fixture(scope="module")
def rt(oracle_lib):
    from robot_mpcs_amd.scenarios import make_scenario
    return dict(Oracle=oracle_lib.Oracle, make_scenario=make_scenario, CENSUS=oracle_lib.CENSUS)


@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3", "cfg4", "boxer", "pointRobot", "panda"])
def test_census_build_reproduces_golden_vectors(rt, name):
    """The vectors test_solve_matches_golden_vectors pins are outputs of the oracle before it counted anything."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    desc = json.loads(str(g["desc"]))
    desc["lb"] = [float(v) for v in desc["lb"]]; desc["ub"] = [float(v) for v in desc["ub"]]
    o = rt["Oracle"](desc)
    for b in range(g["xinit"].shape[0]):
        r = o.solve(g["xinit"][b], g["x0"][b], g["params"][b])
        assert r["exitflag"] == g["exitflag"][b] and r["iters"] == g["iters"][b]
        assert np.array_equal(r["z"], g["z"][b]), (name, b, np.abs(r["z"] - g["z"][b]).max())
        assert r["obj"] == g["obj"][b]
        assert r["census"]["exit"] == r["exitflag"] and r["first"]["exit"] == r["iters"]


@pytest.mark.parametrize("name,seed", [("cfg2", 3), ("cfg3", 3), ("cfg4", 3)])
def test_census_agrees_with_the_trace(rt, name, seed):
    """What the eight trace words show of a solve (accepted halvings per iteration) against the census of the same solve;
    the trace words keep their meaning."""
    sc = rt["make_scenario"](name, B=12, seed=seed)
    o = rt["Oracle"](sc.desc)
    for b in range(12):
        r = o.solve(sc.xinit[b], sc.x0[b], sc.params[b], trace=True)
        assert set(r["census"]) == set(r["first"]) == set(rt["CENSUS"])
        ls = r["trace"][:r["iters"], 7]
        assert r["census"]["ls_max"] == ls.max(initial=0)
        assert r["passes"] >= r["iters"] + 1
        for k, first in r["first"].items():
            assert (first >= 0) == (r["census"][k] != 0) or k == "exit", k
            assert first <= r["iters"]
        # a solve without a null pass pays the first sweep and one sweep per trial point, counted from where each line
        # search began: the halvings themselves plus one (ls_memory == 0: every search began at full length)
        c = r["census"]
        if c["curv_ls_fail"] + c["fact_fail"] + c["cs_retry"] + c["ls_memory"] == 0 and r["exitflag"] >= 0:
            assert r["passes"] == 1 + r["iters"] + int(ls.sum())


def test_cases_are_within_the_stated_sizes():
    assert dc.CASES
    for c in dc.CASES:
        assert c.B <= 16 and 1 <= c.steps <= 5 and 0 <= c.witness < c.B, c
        assert c.mode in ("cold", "warm", "disturbed") and (c.mode != "cold" or c.steps == 1), c
        assert (c.mode == "disturbed") == (c.scale in (0.1, 0.3)), c
        assert c.cls in dc.CLASSES and c.branches and set(c.branches) <= set(dc.BRANCHES), c
        assert not any((c.cls, b) in dc.NOT_APPLICABLE for b in c.branches), c


@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_witness_takes_its_branches_and_is_insensitive_to_rounding(rt, case):
    sc, o, loop = dc.loop_of(rt["make_scenario"], rt["Oracle"], case)
    cpu = loop[-1]["cpu"]
    b = case.witness
    census = cpu["census"][b]
    print(dc.case_id(case), "flag", cpu["exitflag"][b], "iterations", cpu["iters"][b], "passes", cpu["passes"][b], census)
    for k in case.branches:
        assert dc.BRANCHES[k](census), (k, census)
    assert cpu["exitflag"][b] != 0 and cpu["passes"][b] <= dc.MAX_PASSES
    again = dc.witness_solve(o, sc, case, loop[-1])     # (alone, as the filter solves it)
    assert dc.signature(again) == (cpu["exitflag"][b], cpu["iters"][b], cpu["passes"][b], tuple(sorted(census.items())))
    assert dc.rounding_insensitive(o, sc, case, loop[-1])


def test_branch_by_class_table_is_complete():
    have = {(c.cls, b) for c in dc.CASES for b in c.branches}
    pairs = {(cls, b) for cls in dc.CLASSES for b in dc.BRANCHES}
    assert set(dc.NOT_APPLICABLE) <= pairs and set(dc.UNREACHED) <= pairs
    assert not have & set(dc.NOT_APPLICABLE) and not have & set(dc.UNREACHED)
    assert not set(dc.NOT_APPLICABLE) & set(dc.UNREACHED)
    assert all(isinstance(why, str) and "Cfg::" in why for why in dc.NOT_APPLICABLE.values())
    assert len(dc.UNREACHED) <= 3 and all(n >= 256 for n in dc.UNREACHED.values()), dc.UNREACHED
    assert not set(MUST_HAVE) & set(dc.UNREACHED)
    missing = pairs - have - set(dc.NOT_APPLICABLE) - set(dc.UNREACHED)
    assert not missing, sorted(missing)
    # the flags that exclude pairs are those of the model classes: a class's scenarios qualify for what its witnesses take
    assert {cls for cls, _ in have} == set(dc.CLASSES)
