"""The decisions around the step (inst_decide / inst_after_recursion and each kernel family's glue around them) on
every kernel path, on inputs whose oracle solve is KNOWN to take the branch: the witnesses of decision_cases.py
(picked by tools/find_decision_cases.py with the oracle's branch census, pinned on the CPU by
test_decision_census_cpu.py).

Per (witness case, path): a warm-started handle runs the case's closed loop, fed the oracle's inputs step by step (the
loop steps from the oracle's plan, as test_warm_started_closed_loop_matches_oracle does).
  * the witness instance: exit flag and iteration count EQUAL to the oracle's at every step -- no share, no 1 <-> 2
    allowance (the rounding filter on the inputs is what makes that fair) -- and its plan within check_plan's bars
    where the oracle converged;
  * the other instances of the batch, all steps of the loop pooled: check_plan's usual bars;
  * the witness's pass count at the last step (the solve that takes the branches) equals the oracle's, by bracket: the
    loop again with set_pass_budget(p) before the last step -- the witness finishes, same flag and iterations -- and
    again with p - 1 -- flag 0.  A fallback or a retry skipped or taken twice changes passes, not always iterations.
    Every path counts passes as the oracle does (one per horizon evaluation: first sweep, trial points, null passes):
    no path needed a convention of its own;
  * cold witnesses: for each iteration at which one of the case's branches first fired (census), both sides solve with
    max_iter one past it: flag 0, that iteration count, the witness's iterate within check_plan's bars of the oracle's.
Each case prints path, flags, iterations and passes of both sides, and the measured differences.
"""
import numpy as np
import pytest

import decision_cases as dc
from gpu_support import TOL, check_plan

pytestmark = pytest.mark.gpu

SWITCHES = ("RMPC_NO_FUSED", "RMPC_RIC_LANE", "RMPC_NO_MIGRATE", "RMPC_NO_SPEC", "RMPC_ARM_TWO_PARTS")
NOF = {"RMPC_NO_FUSED": "1"}
# path -> (environment at rmpc_create, is_fused, what debug_step reports of the handle's path, ric_first of a solve)
PATHS = {
    "fused": ({}, True, dict(fused="k_fused"), None),    # (under the generated view where the library holds one: _handle)
    "nospec": ({"RMPC_NO_SPEC": "1"}, True, dict(fused="k_fused", generated_view=False), None),
    "pass": (NOF, False, dict(fused="", ric_lane=1), "wave"),
    "lane": (dict(NOF, RMPC_RIC_LANE="2"), False, dict(fused="", ric_lane=2), "lane"),
    "native-pass": ({}, False, dict(fused="", ric_lane=1), "wave"),     # (no switch: the model itself is not fused)
    "arm3": ({}, True, dict(fused="k_fused_arm", arm_parts=3), None),
    "arm2": ({"RMPC_ARM_TWO_PARTS": "1"}, True, dict(fused="k_fused_arm", arm_parts=2), None),
}


VIEWED = ("cfg2",)   # small chains the library holds a generated view of (asserted in _handle; test_spec_gen.py)


def paths_of(c):
    if c.cls == "chain3":
        if c.kw.get("time_horizon", 0) > 32:
            return ("native-pass",)
        return ("fused", "nospec", "pass", "lane") if c.name in VIEWED else ("fused", "pass", "lane")
    if c.cls == "arm":
        return ("native-pass",) if c.name in ("chain4", "chain8") else ("arm3", "arm2", "pass")
    return ("fused", "pass")


PARAMS = [(c, p) for c in dc.CASES for p in paths_of(c)]


def _set_env(monkeypatch, env):
    """The switches a handle reads once, at rmpc_create: those of the path and no others."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def rt():
    import __graft_entry__ as g
    g.build()
    from oracle.oracle import Oracle
    from robot_mpcs_amd._lib import Solver, spec_for
    from robot_mpcs_amd.scenarios import make_scenario
    return dict(Oracle=Oracle, Solver=Solver, make_scenario=make_scenario, spec_for=spec_for)


def _handle(rt, sc, c, path):
    env, fused, want, _ = PATHS[path]
    s = rt["Solver"](sc.desc, max_batch=c.B)
    assert s.is_fused() == fused, path
    d = s.debug_step(sc.xinit, sc.x0, sc.params)     # (the path the switches selected, as the Newton-step tests read it)
    for key, v in want.items():
        assert d["path"][key] == v, (path, key, d["path"])
    view = rt["spec_for"](sc.desc)   # ("" when the library holds no generated view of this model)
    assert view != "" or not (c.cls == "chain3" and c.name in VIEWED), (c.name, view)
    assert d["path"]["generated_view"] == (s.spec_name() != "") == (view != "" and path != "nospec"), (path, view, d["path"])
    return s


def _run(s, sc, loop, budget=0):
    """The loop on the handle from a forgotten warm start; ``budget``: set_pass_budget before the last step."""
    s.set_pass_budget(0)
    s.set_warm_start(False); s.set_warm_start(True)
    out = []
    for t, step in enumerate(loop):
        if t == len(loop) - 1:
            s.set_pass_budget(budget)
        out.append(s.solve(step["x"], step["x0"], sc.params))
    s.set_pass_budget(0)
    return out


def _plan_diff(gz, cz, nxs):
    """(whole plan, applied control) differences over check_plan's scales."""
    return (np.abs(gz - cz).max() / max(1.0, np.abs(cz).max()),
            np.abs(gz[0, nxs:] - cz[0, nxs:]).max() / max(1.0, np.abs(cz[0, nxs:]).max()))


@pytest.mark.parametrize("case,path", PARAMS, ids=["%s-%s" % (dc.case_id(c), p) for c, p in PARAMS])
def test_decisions_match_oracle_on_witness(rt, case, path, monkeypatch):
    _set_env(monkeypatch, PATHS[path][0])
    sc, o, loop = dc.loop_of(rt["make_scenario"], rt["Oracle"], case)
    nxs, b, last = o.nx + o.ns, case.witness, len(loop) - 1
    s = _handle(rt, sc, case, path)
    got = _run(s, sc, loop)
    lp = s.last_solve_path()
    assert lp["fused"] == PATHS[path][1] and (PATHS[path][3] is None or lp["ric_first"] == PATHS[path][3]), lp
    others = np.arange(case.B) != b
    for t, (g, step) in enumerate(zip(got, loop)):
        cpu = step["cpu"]
        print("%s %s step %d witness: flag gpu %d cpu %d, iterations gpu %d cpu %d, passes cpu %d" % (
            dc.case_id(case), path, t, g["exitflag"][b], cpu["exitflag"][b], g["iters"][b], cpu["iters"][b], cpu["passes"][b]))
        assert g["exitflag"][b] == cpu["exitflag"][b] and g["iters"][b] == cpu["iters"][b], (t, g["exitflag"], cpu["exitflag"], g["iters"], cpu["iters"])
        if cpu["exitflag"][b] in (1, 2):
            dz, du = _plan_diff(g["z"][b], cpu["z"][b], nxs)
            print("    plan difference %.2e, applied control %.2e (bar %.0e)" % (dz, du, TOL))
            assert dz <= TOL and du <= TOL, (t, dz, du)
    pool = lambda side, key: np.concatenate([r[key][others] for r in side])
    cpus = [step["cpu"] for step in loop]
    check_plan({k: pool(got, k) for k in ("exitflag", "iters", "z", "kkt")}, {k: pool(cpus, k) for k in ("exitflag", "iters", "z")}, nxs)
    # ---- the witness's passes at the last step, bracketed by the pass budget ----
    p, flag, iters = int(loop[last]["cpu"]["passes"][b]), loop[last]["cpu"]["exitflag"][b], loop[last]["cpu"]["iters"][b]
    at = _run(s, sc, loop, budget=p)[last]
    assert at["exitflag"][b] == flag and at["iters"][b] == iters, (p, at["exitflag"][b], at["iters"][b])
    below = _run(s, sc, loop, budget=p - 1)[last] if p >= 2 else None
    print("    passes: finished with a budget of %d (flag %d); with %d: flag %s" % (p, at["exitflag"][b], p - 1, None if below is None else below["exitflag"][b]))
    assert below is None or below["exitflag"][b] == 0, (p, below["exitflag"][b])
    s.close()


COLD = [(c, p) for c, p in PARAMS if c.mode == "cold"]


@pytest.mark.parametrize("case,path", COLD, ids=["%s-%s" % (dc.case_id(c), p) for c, p in COLD])
def test_iterate_after_the_branch_matches_oracle(rt, case, path, monkeypatch):
    """Cold witnesses, cut one iteration past the first firing of each of the case's branches."""
    _set_env(monkeypatch, PATHS[path][0])
    sc, o, loop = dc.loop_of(rt["make_scenario"], rt["Oracle"], case)
    nxs, b = o.nx + o.ns, case.witness
    first, iters = loop[0]["cpu"]["first"][b], int(loop[0]["cpu"]["iters"][b])
    cuts = sorted({first[dc.FIRST_OF.get(k, k)] + 1 for k in case.branches} - {0})
    cuts = [f for f in cuts if f < iters]    # (at its last iteration the solve stops by itself: the loop test above)
    assert cuts, (case, first)
    for f in cuts:
        desc = dict(sc.desc, options=dict(sc.desc["options"], max_iter=f))
        r = rt["Oracle"](desc).solve_warm(sc.xinit[b], sc.x0[b], sc.params[b])
        s = rt["Solver"](desc, max_batch=case.B)
        assert s.is_fused() == PATHS[path][1]
        g = s.solve(sc.xinit, sc.x0, sc.params)
        s.close()
        took = [k for k in case.branches if first[dc.FIRST_OF.get(k, k)] + 1 == f]
        dz, du = _plan_diff(g["z"][b], r["z"], nxs)
        print("%s %s cut at %d (%s): flag gpu %d cpu %d, iterations gpu %d cpu %d, iterate difference %.2e, first control %.2e (bar %.0e)" % (
            dc.case_id(case), path, f, " ".join(took), g["exitflag"][b], r["exitflag"], g["iters"][b], r["iters"], dz, du, TOL))
        assert r["exitflag"] == 0 and r["iters"] == f
        assert g["exitflag"][b] == 0 and g["iters"][b] == f
        assert dz <= TOL and du <= TOL, (f, dz, du)
