"""Witnesses of the solver's decision branches and the closed loop that reaches them; shared by
test_decision_census_cpu.py, test_gpu_decision_branches.py and tools/find_decision_cases.py.

A case is a small closed loop: a scenario (``make_scenario(name, B, seed, **kw)`` plus option overrides), a mode, a number
of control steps, and ONE witness instance whose oracle solve at the last step takes the branches listed (the oracle's
branch census, oracle/rmpc_oracle.h ORC_CEN_*).  Modes:
  cold       the scenario as it is, one solve;
  warm       previous plan shifted, the oracle's own multipliers, plant = the model's discrete map;
  disturbed  as warm, the measured state moved by ``scale`` times a unit-normal vector drawn from the case's seed, the same
             vector at every run.
The witnesses were picked by tools/find_decision_cases.py: cheapest first (fewest passes, at most 60), and only instances
whose flag, iteration count, pass count and census do not move under relative perturbations of 1e-8 of the inputs
(``perturbed`` below) -- the device's multipliers differ from the oracle's in the last digits, and a crawl amplifies that.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

MAX_PASSES = 60          # a witness finishes within this many passes
PERTURBATIONS = 8        # rounding filter: draws ...
PERTURB_REL = 1e-8       # ... of this relative size, on xinit, x0 and the warm multipliers

# the branch axis of the table: name -> predicate on the census of a solve (oracle.CENSUS)
BRANCHES = {
    "gn_backtrack": lambda c: c["gn_backtrack"] > 0,
    "ls_memory": lambda c: c["ls_memory"] > 0,
    "curv_halved": lambda c: c["curv_halved"] > 0,
    "curv_ls_fail": lambda c: c["curv_ls_fail"] > 0,
    "fact_fail": lambda c: c["fact_fail"] > 0,
    "cs_retry": lambda c: c["cs_retry"] > 0,
    "cs_kept": lambda c: c["cs_kept"] > 0,
    "cs_doubled": lambda c: c["cs_doubled"] > 0,
    "cs_exhausted": lambda c: c["cs_exhausted"] > 0,
    "skip": lambda c: c["skip"] > 0,
    "back4": lambda c: c["back_max"] >= 4,
    "latch_set": lambda c: c["latch_set"] > 0,
    "latch_released": lambda c: c["latch_released"] > 0,
    "restart": lambda c: c["restart"] > 0,
    "rho_raised": lambda c: c["rho_raised"] > 0,
    "stall_reset": lambda c: c["stall_reset"] > 0,
    "flag1": lambda c: c["exit"] == 1,
    "flag2": lambda c: c["exit"] == 2,
    "flag-7": lambda c: c["exit"] == -7,
}
# the census counter whose first-iteration entry dates a branch (cold witnesses: the cut at that iteration)
FIRST_OF = {"back4": "back_max", "flag1": "exit", "flag2": "exit", "flag-7": "exit"}

# model classes: the decision logic is compiled per class (Cfg flags of csrc/rmpc_solver.hpp)
CLASSES = {
    "chain3": "small holonomic chain without slack (cfg2, chain2, wc_point): Cfg::CURV + CSCALE + BACKOFF",
    "point_slack": "point robot with the slack variable (cfg2, slack=True): no curvature terms",
    "unicycle": "diff-drive base with and without slack (cfg3, boxer, wc_boxer, wc_boxer_slack): Cfg::DDCURV + BACKOFF",
    "arm": "arms (cfg4, chain4, chain5, chain6, chain8): Cfg::CURV + FKCURV, the latch and its release",
}
_CURV = ("curv_halved", "curv_ls_fail", "fact_fail")
_CS = ("cs_retry", "cs_kept", "cs_doubled", "cs_exhausted")
_BACK = ("skip", "back4")
_LATCH = ("latch_set", "latch_released")
# pairs that cannot occur, with the Cfg flag that excludes them
NOT_APPLICABLE = dict(
    [(("chain3", b), "not Cfg::FKCURV (Cfg::BACKOFF instead of the latch)") for b in _LATCH]
    + [(("point_slack", b), "neither Cfg::CURV nor Cfg::DDCURV (slack variable: no curvature step)") for b in _CURV + _CS + _BACK + _LATCH]
    + [(("unicycle", b), "not Cfg::CSCALE") for b in _CS]
    + [(("unicycle", b), "not Cfg::FKCURV (Cfg::BACKOFF instead of the latch)") for b in _LATCH]
    + [(("arm", b), "not Cfg::CSCALE") for b in _CS]
    + [(("arm", b), "not Cfg::BACKOFF (the latch instead)") for b in _BACK])

Case = namedtuple("Case", "cls name kw opts seed B steps mode scale witness branches")
# opts: overrides of desc["options"] (mu0); witness: index of the witness instance; branches: what its solve at the LAST
# step takes.  Filled from the output of tools/find_decision_cases.py.
CASES = [
    Case('arm', 'cfg4', {}, {}, 8, 16, 4, 'disturbed', 0.1, 1, ('curv_ls_fail', 'flag1', 'gn_backtrack', 'latch_released', 'latch_set', 'ls_memory', 'rho_raised')),   # 17 passes
    Case('arm', 'chain5', {}, {}, 8, 16, 5, 'disturbed', 0.3, 13, ('curv_halved', 'flag-7')),   # 19 passes
    Case('arm', 'chain5', {}, {'mu0': 0.01}, 3, 16, 1, 'cold', 0.0, 2, ('fact_fail',)),   # 13 passes
    Case('arm', 'cfg4', {}, {}, 5, 16, 3, 'disturbed', 0.3, 10, ('restart',)),   # 20 passes
    Case('arm', 'chain4', {}, {}, 7, 16, 4, 'disturbed', 0.1, 5, ('curv_ls_fail', 'flag1', 'gn_backtrack', 'latch_released', 'latch_set', 'ls_memory', 'rho_raised')),   # 17 passes (+dense)
    Case('arm', 'chain8', {}, {}, 10, 16, 4, 'disturbed', 0.3, 2, ('curv_halved', 'flag-7')),   # 26 passes (+dense)
    Case('arm', 'chain8', {}, {}, 8, 16, 2, 'disturbed', 0.3, 6, ('stall_reset',)),   # 12 passes (+dense)
    Case('arm', 'chain4', {}, {'mu0': 0.01}, 1, 16, 1, 'cold', 0.0, 7, ('fact_fail',)),   # 13 passes (+dense)
    Case('arm', 'chain4', {}, {}, 5, 16, 2, 'disturbed', 0.3, 3, ('restart',)),   # 20 passes (+dense)
    Case('chain3', 'cfg2', {}, {}, 3, 16, 2, 'warm', 0.0, 5, ('back4', 'cs_doubled', 'cs_kept', 'cs_retry', 'curv_halved', 'curv_ls_fail', 'flag2', 'gn_backtrack', 'ls_memory', 'rho_raised', 'skip', 'stall_reset')),   # 55 passes
    Case('chain3', 'cfg2', {}, {'mu0': 0.01}, 7, 16, 1, 'cold', 0.0, 1, ('restart',)),   # 20 passes (under the generated view)
    Case('chain3', 'chain2', {}, {'mu0': 0.01}, 5, 16, 1, 'cold', 0.0, 4, ('cs_exhausted', 'fact_fail', 'flag1')),   # 18 passes
    Case('chain3', 'chain2', {}, {}, 2, 16, 3, 'disturbed', 0.3, 6, ('flag-7',)),   # 17 passes
    Case('chain3', 'chain2', {}, {'mu0': 0.01}, 5, 16, 1, 'cold', 0.0, 11, ('restart',)),   # 20 passes
    Case('chain3', 'cfg2', {'time_horizon': 40}, {'mu0': 0.01}, 6, 16, 1, 'cold', 0.0, 13, ('back4', 'cs_doubled', 'cs_exhausted', 'cs_kept', 'cs_retry', 'fact_fail', 'flag1', 'restart', 'skip')),   # 26 passes (+N40)
    Case('chain3', 'cfg2', {'time_horizon': 40}, {}, 2, 16, 4, 'warm', 0.0, 0, ('curv_ls_fail', 'gn_backtrack', 'ls_memory', 'rho_raised')),   # 12 passes (+N40)
    Case('chain3', 'cfg2', {'time_horizon': 40}, {}, 1, 16, 4, 'disturbed', 0.1, 9, ('curv_halved',)),   # 6 passes (+N40)
    Case('chain3', 'cfg2', {'time_horizon': 40}, {}, 8, 16, 5, 'disturbed', 0.3, 11, ('flag-7',)),   # 13 passes (+N40)
    Case('point_slack', 'cfg2', {'slack': True}, {'mu0': 0.01}, 7, 16, 1, 'cold', 0.0, 12, ('flag1', 'gn_backtrack', 'ls_memory', 'restart', 'rho_raised', 'stall_reset')),   # 35 passes
    Case('point_slack', 'cfg2', {'slack': True}, {}, 1, 16, 3, 'disturbed', 0.3, 13, ('flag2',)),   # 13 passes
    Case('unicycle', 'cfg3', {}, {}, 5, 16, 2, 'warm', 0.0, 13, ('curv_halved', 'curv_ls_fail', 'flag1', 'gn_backtrack', 'ls_memory', 'rho_raised', 'skip', 'stall_reset')),   # 14 passes
    Case('unicycle', 'cfg3', {}, {'mu0': 0.01}, 4, 16, 1, 'cold', 0.0, 2, ('back4', 'fact_fail')),   # 17 passes
    Case('unicycle', 'cfg3', {}, {}, 6, 16, 2, 'disturbed', 0.3, 0, ('restart',)),   # 21 passes
    Case('unicycle', 'cfg3', {}, {}, 3, 16, 5, 'warm', 0.0, 13, ('flag2',)),   # 25 passes
    Case('unicycle', 'wc_boxer_slack', {}, {'mu0': 0.01}, 3, 16, 1, 'cold', 0.0, 13, ('back4', 'curv_halved', 'curv_ls_fail', 'flag2', 'gn_backtrack', 'ls_memory', 'rho_raised', 'skip')),   # 37 passes (+slack)
    Case('unicycle', 'wc_boxer_slack', {}, {'mu0': 0.01}, 1, 16, 1, 'cold', 0.0, 6, ('fact_fail', 'flag1', 'restart', 'stall_reset')),   # 41 passes (+slack)
]
# (class, branch): instances searched without a rounding-insensitive witness
UNREACHED = {
    ('point_slack', 'flag-7'): 3264,   # (never seen, rounding filter aside)
    ('unicycle', 'flag-7'): 13056,   # (never seen, rounding filter aside)
    ('arm', 'flag2'): 16320,   # (never seen, rounding filter aside)
}


def case_id(c):
    return "%s-%s-s%d-%s%s-w%d" % (c.cls, c.name + "".join("-%s%s" % (k[0], v) for k, v in sorted(c.kw.items()))
                                   + "".join("-%s%g" % (k, v) for k, v in sorted(c.opts.items())), c.seed, c.mode,
                                   ("%g" % c.scale) if c.mode == "disturbed" else "", c.witness)


def scenario_of(make_scenario, c, kw_extra=None):
    """The case's scenario, its options overridden (the overrides reach the oracle and the library through the descriptor)."""
    sc = make_scenario(c.name, B=c.B, seed=c.seed, **dict(c.kw, **(kw_extra or {})))
    sc.desc["options"] = dict(sc.desc["options"], **c.opts)
    return sc


def disturbance(c, nx):
    """[steps, B, nx]: what is added to the measured state before step t >= 1 (zero unless the mode is ``disturbed``)."""
    if c.mode != "disturbed":
        return np.zeros((c.steps, c.B, nx))
    rng = np.random.default_rng(zlib.crc32(repr((c.name, c.seed, "disturbance")).encode()))
    return c.scale * rng.standard_normal((c.steps, c.B, nx))


def perturbed(rng, a, rel=PERTURB_REL):
    a = np.asarray(a, dtype=np.float64)
    return a * (1.0 + rel * rng.uniform(-1.0, 1.0, a.shape))


def failed_duals(o, mu0):
    """What a failed solve leaves behind for the next one, on both sides: zero multipliers and mu0."""
    return (np.zeros((o.N, o.m)), np.zeros((o.N, o.nx)), mu0 / 1000.0)


def oracle_loop(sc, o, c):
    """The closed loop on the oracle: a list with one entry per control step -- the inputs of the step (``x``, ``x0``,
    ``duals``: what each instance starts from) and ``cpu``, Oracle.solve_each of them.  The loop steps from the oracle's
    plan, so a device handle fed the same ``x`` / ``x0`` step by step solves the same problems."""
    nxs, mu0 = o.nx + o.ns, sc.desc["options"]["mu0"]
    dist = disturbance(c, o.nx)
    x, x0 = sc.xinit.copy(), sc.x0.copy()
    duals = None
    out = []
    for t in range(c.steps):
        cpu = o.solve_each(x, x0, sc.params, duals)
        out.append(dict(x=x.copy(), x0=x0.copy(), duals=duals, cpu=cpu))
        duals = [cpu["duals"][b] if cpu["exitflag"][b] >= 0 else failed_duals(o, mu0) for b in range(c.B)]
        if t + 1 < c.steps:
            z = cpu["z"]
            x = np.array([o.dynamics(x[b], z[b, 0, nxs:]) for b in range(c.B)]) + dist[t + 1]
            x0 = np.concatenate([z[:, 1:], z[:, -1:]], axis=1)
    return out


def witness_solve(o, sc, c, step, rng=None):
    """The witness's solve of one step again, alone; ``rng``: with the rounding filter's perturbation of its inputs."""
    b = c.witness
    x, x0, duals = step["x"][b], step["x0"][b], None if step["duals"] is None else step["duals"][b]
    if rng is not None:
        x, x0 = perturbed(rng, x), perturbed(rng, x0)
        if duals is not None:
            duals = (perturbed(rng, duals[0]), perturbed(rng, duals[1]), duals[2])
    return o.solve_warm(x, x0, sc.params[b], duals)


def signature(r):
    """What the rounding filter compares."""
    return (r["exitflag"], r["iters"], r["passes"], tuple(sorted(r["census"].items())))


def rounding_insensitive(o, sc, c, step, draws=PERTURBATIONS):
    rng = np.random.default_rng(zlib.crc32(repr((c.name, c.seed, c.witness, "filter")).encode()))
    want = signature(witness_solve(o, sc, c, step))
    return all(signature(witness_solve(o, sc, c, step, rng)) == want for _ in range(draws))


@functools.lru_cache(maxsize=None)
def _loop_cached(make_scenario, Oracle, c_key):
    c = CASES[c_key]
    sc = scenario_of(make_scenario, c)
    o = Oracle(sc.desc)
    return sc, o, oracle_loop(sc, o, c)


def loop_of(make_scenario, Oracle, c):
    """(scenario, oracle, oracle_loop) of a committed case, computed once per session."""
    return _loop_cached(make_scenario, Oracle, CASES.index(c))
