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
    max_iter one past it: flag 0, that iteration count, the witness's iterate within check_plan's bars of the oracle's;
  * the witnesses under option sets off the defaults (decision_cases.OPTION_SETS: the acceptable window, the benchmark's
    options, a small line-search cap, loose tolerances) go through the same two tests; where the witness ends the last step
    with flag 0 or -8 its returned iterate is compared like a cut's (a line search that runs out returns the current
    iterate on both sides);
  * the edge witnesses (decision_cases.EDGES), one handle per option variant: max_iter equal to the iteration at which
    the witness converges (or reaches the acceptable level) ends with that flag, one less with flag 0 -- the order of
    the stop tests in inst_decide; the acceptable window switched off and one iteration longer;
  * wherever a witness is compared at flag 0, -8 or a cut: the reported objective to OBJ_RTOL and the reported residual
    kkt against the oracle's max(res_stat, res_eq, res_ineq, res_comp) to decision_cases.KKT_REL, eight times the
    oracle's own movement under the rounding filter's perturbations (measured on the CPU).
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


def _check_reported(label, g, b, obj, kkt):
    """The numbers a caller is told beside the plan: objective and KKT residual of the returned iterate."""
    dobj = abs(g["obj"][b] - obj) / abs(obj)
    dk = abs(g["kkt"][b] - kkt) / kkt if kkt >= dc.KKT_FLOOR else None
    print("    %s: obj gpu %.12e cpu %.12e (relative %.2e, bar %.0e); kkt gpu %.6e cpu %.6e (relative %s, bar %.2e)" % (
        label, g["obj"][b], obj, dobj, dc.OBJ_RTOL, g["kkt"][b], kkt, "below the floor, not compared" if dk is None else "%.2e" % dk, dc.KKT_REL))
    assert dobj <= dc.OBJ_RTOL, (label, dobj)
    assert dk is None or dk <= dc.KKT_REL, (label, dk)


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
        if t == last and cpu["exitflag"][b] in (0, -8):     # (the returned iterate, like a cut's, and what is reported of it)
            dz, du = _plan_diff(g["z"][b], cpu["z"][b], nxs)
            print("    iterate difference %.2e, first control %.2e (bar %.0e)" % (dz, du, TOL))
            assert dz <= TOL and du <= TOL, (t, dz, du)
            _check_reported("step %d" % t, g, b, cpu["obj"][b], cpu["kkt"][b])
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
    if flag == 0 and below is not None:
        # (a witness that ends with flag 0 by itself: one pass short it has not reached its last iteration either)
        print("    iterations with a budget of %d: %d (with %d: %d)" % (p - 1, below["iters"][b], p, at["iters"][b]))
        assert below["iters"][b] < iters, (p, below["iters"][b], iters)
    s.close()


COLD = [(c, p) for c, p in PARAMS if dc.has_cuts(c)]     # (cold, and a branch that is not dated by the exit)


@pytest.mark.parametrize("case,path", COLD, ids=["%s-%s" % (dc.case_id(c), p) for c, p in COLD])
def test_iterate_after_the_branch_matches_oracle(rt, case, path, monkeypatch):
    """Cold witnesses, cut one iteration past the first firing of each of the case's branches."""
    _set_env(monkeypatch, PATHS[path][0])
    sc, o, loop = dc.loop_of(rt["make_scenario"], rt["Oracle"], case)
    nxs, b = o.nx + o.ns, case.witness
    first, iters = loop[0]["cpu"]["first"][b], int(loop[0]["cpu"]["iters"][b])
    cuts = dc.cut_iterations(case, first, iters)    # (at its last iteration the solve stops by itself: the loop test above)
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
        _check_reported("cut at %d" % f, g, b, r["obj"], dc.kkt_of(r))


def _edge_params(kind):
    return [(e, p) for e in dc.EDGES if e.kind == kind for p in paths_of(dc.CASES[e.case])]


def _check_edge(rt, edge, path, monkeypatch):
    """Every option variant of the edge through a handle of its own on the path, fed the case's inputs step by step:
    flag and iterations of the witness equal to the oracle's at every step, plan (flag 1, 2) within TOL, and at the last
    step -- the solve the rounding filter vouches for -- the iterate and the reported numbers where the oracle stops
    with 0 or -8."""
    _set_env(monkeypatch, PATHS[path][0])
    (sc, o, loop), variants = dc.edge_loops(rt["make_scenario"], rt["Oracle"], edge)
    case = dc.CASES[edge.case]
    nxs, b = o.nx + o.ns, case.witness
    results = {}
    for (label, cv, scv, ov, lp), want in zip(variants, edge.expect):
        s = _handle(rt, scv, cv, path)
        got = _run(s, scv, lp)
        lpath = s.last_solve_path()
        s.close()
        assert lpath["fused"] == PATHS[path][1] and (PATHS[path][3] is None or lpath["ric_first"] == PATHS[path][3]), lpath
        for t, (g, step) in enumerate(zip(got, lp)):
            cpu = step["cpu"]
            dz, du = _plan_diff(g["z"][b], cpu["z"][b], nxs)
            print("%s %s %s %s step %d witness: flag gpu %d cpu %d, iterations gpu %d cpu %d, passes cpu %d, plan or iterate difference %.2e, first control %.2e (bar %.0e)" % (
                dc.edge_id(edge), path, label, cv.opts, t, g["exitflag"][b], cpu["exitflag"][b], g["iters"][b], cpu["iters"][b], cpu["passes"][b], dz, du, TOL))
            assert g["exitflag"][b] == cpu["exitflag"][b] and g["iters"][b] == cpu["iters"][b], (label, t, g["exitflag"], cpu["exitflag"], g["iters"], cpu["iters"])
            if cpu["exitflag"][b] in (1, 2) or (t == len(lp) - 1 and cpu["exitflag"][b] in (0, -8)):
                assert dz <= TOL and du <= TOL, (label, t, dz, du)
            if t == len(lp) - 1 and cpu["exitflag"][b] in (0, -8):
                _check_reported("%s step %d" % (label, t), g, b, cpu["obj"][b], cpu["kkt"][b])
        last = dc.result_of(lp[-1]["cpu"], b)
        assert last == want, (label, last, want)      # (the oracle's side is what the CPU test pinned)
        results[label] = (int(got[-1]["exitflag"][b]), int(got[-1]["iters"][b]))
    return results


@pytest.mark.parametrize("edge,path", _edge_params("max_iter"), ids=["%s-%s" % (dc.edge_id(e), p) for e, p in _edge_params("max_iter")])
def test_stop_order_at_the_iteration_limit(rt, edge, path, monkeypatch):
    """max_iter = n, the iteration at which the witness converges (flag 1) or reaches the acceptable level (flag 2): that
    flag and n iterations, not flag 0 -- converged, then acceptable, then the iteration limit; max_iter = n - 1: flag 0 and
    n - 1 iterations."""
    res = _check_edge(rt, edge, path, monkeypatch)
    assert res["at"] == (edge.flag, edge.n) and res["below"] == (0, edge.n - 1), res


@pytest.mark.parametrize("edge,path", _edge_params("acc_iters"), ids=["%s-%s" % (dc.edge_id(e), p) for e, p in _edge_params("acc_iters")])
def test_acceptable_window_edges(rt, edge, path, monkeypatch):
    """A witness that ends with flag 2 under acc_iters = k: with acc_iters = 0 the window is off (never flag 2), with
    k + 1 it ends as the oracle says."""
    res = _check_edge(rt, edge, path, monkeypatch)
    assert res["off"][0] != 2, res
