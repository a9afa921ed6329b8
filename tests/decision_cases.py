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
Beside the witnesses at the default options: witnesses under option sets off the defaults (OPTION_SETS; their results
pinned in EXPECT), edge witnesses derived from the cases by rule (EDGES: max_iter at the iteration a solve stops by
itself, the acceptable window off and one longer), and the bar of the reported residual (KKT_REL).
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
    # reached under option sets off the defaults only (OPTION_SETS below)
    "flag0": lambda c: c["exit"] == 0,
    "flag-8": lambda c: c["exit"] == -8,
    # converged under LOOSE in strictly fewer iterations than the same inputs take at the default tolerances
    # (``default_iters``: census_view below; absent from a plain census, so never true of one)
    "loose_flag1": lambda c: c["exit"] == 1 and c.get("default_iters", -1) > c.get("iters", 1 << 30),
}
# the census counter whose first-iteration entry dates a branch (cold witnesses: the cut at that iteration)
FIRST_OF = {"back4": "back_max", "flag1": "exit", "flag2": "exit", "flag-7": "exit", "flag0": "exit", "flag-8": "exit",
            "loose_flag1": "exit"}

# Option sets off the defaults.  ACC: the acceptable stop after ONE stagnant iteration at a coarse
# objective bar; ACC_OFF: no acceptable stop; BENCH: what bench.py runs; LS: the small line-search cap rmpc.h advertises
# for real-time loops; LOOSE: every tolerance of the converged stop moved (tol_comp also moves the barrier floor
# 0.1 tol_comp and the release of a held barrier).
ACC = {"acc_iters": 1, "acc_obj_tol": 1e-4}
ACC_OFF = {"acc_iters": 0}
BENCH = {"max_iter": 20, "acc_iters": 3}
LS = {"ls_max": 2}
LOOSE = {"tol_stat": 1e-3, "tol_eq": 1e-5, "tol_ineq": 1e-5, "tol_comp": 1e-3}
OPTION_SETS = {"ACC": ACC, "ACC_OFF": ACC_OFF, "BENCH": BENCH, "LS": LS, "LOOSE": LOOSE}
# (branch, option sets under which its witnesses are searched): one witness each per class, per recursion family of the
# arms and at the horizon of 40 stages
OPTION_BRANCHES = {"flag2": ("ACC", "BENCH"), "flag0": ("BENCH",), "flag-8": ("LS",), "loose_flag1": ("LOOSE",)}
DEFAULT_ONLY = [k for k in BRANCHES if k not in ("flag0", "flag-8", "loose_flag1")]    # what the default options reach

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
# under the option sets above (tools/find_decision_cases.py --part options: four seeds, per class -- per recursion family
# of the arms, and at the horizon of 40 stages -- and exit the cheapest witness over the sets that reach it; last, per
# class without a cold flag-2 case at the default options, the cheapest cold one: the max_iter edge below wants one; and
# per class the cheapest flag -8 exit after an accepted step ("later"): the cheapest of all fail their first line search)
CASES += [
    Case('arm', 'cfg4', {}, {'acc_iters': 1, 'acc_obj_tol': 0.0001}, 1, 16, 2, 'warm', 0.0, 13, ('flag2',)),   # 4 passes, ACC
    Case('arm', 'cfg4', {}, {'max_iter': 20, 'acc_iters': 3}, 1, 16, 2, 'disturbed', 0.1, 8, ('flag0',)),   # 21 passes, BENCH
    Case('arm', 'cfg4', {}, {'ls_max': 2}, 1, 16, 3, 'disturbed', 0.3, 0, ('flag-8',)),   # 4 passes, LS
    Case('arm', 'chain6', {}, {'tol_stat': 0.001, 'tol_eq': 1e-05, 'tol_ineq': 1e-05, 'tol_comp': 0.001}, 2, 16, 4, 'disturbed', 0.3, 14, ('loose_flag1',)),   # 5 passes, LOOSE
    Case('arm', 'chain4', {}, {'acc_iters': 1, 'acc_obj_tol': 0.0001}, 2, 16, 2, 'disturbed', 0.1, 0, ('flag2',)),   # 4 passes, ACC (+dense)
    Case('arm', 'chain4', {}, {'max_iter': 20, 'acc_iters': 3}, 1, 16, 2, 'disturbed', 0.3, 8, ('flag0',)),   # 21 passes, BENCH (+dense)
    Case('arm', 'chain8', {}, {'ls_max': 2}, 2, 16, 4, 'disturbed', 0.3, 4, ('flag-8',)),   # 4 passes, LS (+dense)
    Case('arm', 'chain4', {}, {'tol_stat': 0.001, 'tol_eq': 1e-05, 'tol_ineq': 1e-05, 'tol_comp': 0.001}, 3, 16, 5, 'disturbed', 0.1, 0, ('loose_flag1',)),   # 5 passes, LOOSE (+dense)
    Case('chain3', 'wc_point', {}, {'acc_iters': 1, 'acc_obj_tol': 0.0001}, 1, 16, 2, 'disturbed', 0.1, 14, ('flag2',)),   # 4 passes, ACC
    Case('chain3', 'cfg2', {}, {'max_iter': 20, 'acc_iters': 3}, 4, 16, 1, 'cold', 0.0, 8, ('flag0',)),   # 21 passes, BENCH
    Case('chain3', 'cfg2', {}, {'ls_max': 2}, 1, 16, 3, 'disturbed', 0.1, 12, ('flag-8',)),   # 4 passes, LS
    Case('chain3', 'wc_point', {}, {'tol_stat': 0.001, 'tol_eq': 1e-05, 'tol_ineq': 1e-05, 'tol_comp': 0.001}, 1, 16, 2, 'warm', 0.0, 2, ('loose_flag1',)),   # 5 passes, LOOSE
    Case('chain3', 'cfg2', {'time_horizon': 40}, {'acc_iters': 1, 'acc_obj_tol': 0.0001}, 2, 16, 2, 'disturbed', 0.1, 1, ('flag2',)),   # 4 passes, ACC (+N40)
    Case('chain3', 'cfg2', {'time_horizon': 40}, {'max_iter': 20, 'acc_iters': 3}, 2, 16, 1, 'cold', 0.0, 5, ('flag0',)),   # 21 passes, BENCH (+N40)
    Case('chain3', 'cfg2', {'time_horizon': 40}, {'ls_max': 2}, 1, 16, 3, 'disturbed', 0.1, 9, ('flag-8',)),   # 4 passes, LS (+N40)
    Case('chain3', 'cfg2', {'time_horizon': 40}, {'tol_stat': 0.001, 'tol_eq': 1e-05, 'tol_ineq': 1e-05, 'tol_comp': 0.001}, 3, 16, 5, 'warm', 0.0, 14, ('loose_flag1',)),   # 6 passes, LOOSE (+N40)
    Case('point_slack', 'cfg2', {'slack': True}, {'acc_iters': 1, 'acc_obj_tol': 0.0001}, 4, 16, 2, 'warm', 0.0, 8, ('flag2',)),   # 4 passes, ACC
    Case('point_slack', 'cfg2', {'slack': True}, {'max_iter': 20, 'acc_iters': 3}, 1, 16, 2, 'disturbed', 0.1, 10, ('flag0',)),   # 21 passes, BENCH
    Case('point_slack', 'cfg2', {'slack': True}, {'ls_max': 2}, 1, 16, 1, 'cold', 0.0, 14, ('flag-8',)),   # 4 passes, LS
    Case('point_slack', 'cfg2', {'slack': True}, {'tol_stat': 0.001, 'tol_eq': 1e-05, 'tol_ineq': 1e-05, 'tol_comp': 0.001}, 2, 16, 2, 'disturbed', 0.1, 6, ('loose_flag1',)),   # 6 passes, LOOSE
    Case('unicycle', 'cfg3', {}, {'acc_iters': 1, 'acc_obj_tol': 0.0001}, 1, 16, 2, 'warm', 0.0, 1, ('flag2',)),   # 4 passes, ACC
    Case('unicycle', 'cfg3', {}, {'max_iter': 20, 'acc_iters': 3}, 3, 16, 1, 'cold', 0.0, 5, ('flag0',)),   # 22 passes, BENCH
    Case('unicycle', 'cfg3', {}, {'ls_max': 2}, 1, 16, 2, 'warm', 0.0, 7, ('flag-8',)),   # 4 passes, LS
    Case('unicycle', 'boxer', {}, {'tol_stat': 0.001, 'tol_eq': 1e-05, 'tol_ineq': 1e-05, 'tol_comp': 0.001}, 2, 16, 4, 'disturbed', 0.3, 2, ('loose_flag1',)),   # 4 passes, LOOSE
    Case('chain3', 'wc_point', {}, {'acc_iters': 1, 'acc_obj_tol': 0.0001}, 2, 16, 1, 'cold', 0.0, 7, ('flag2',)),   # 9 passes, ACC cold
    Case('point_slack', 'cfg2', {'slack': True}, {'acc_iters': 1, 'acc_obj_tol': 0.0001}, 1, 16, 1, 'cold', 0.0, 0, ('flag2',)),   # 12 passes, ACC cold
    Case('arm', 'cfg4', {}, {'acc_iters': 1, 'acc_obj_tol': 0.0001}, 1, 16, 1, 'cold', 0.0, 12, ('flag2',)),   # 10 passes, ACC cold
    Case('chain3', 'cfg2', {'time_horizon': 40}, {'ls_max': 2}, 2, 16, 3, 'disturbed', 0.3, 10, ('flag-8',)),   # 5 passes, LS later
    Case('point_slack', 'cfg2', {'slack': True}, {'ls_max': 2}, 3, 16, 2, 'disturbed', 0.1, 3, ('flag-8',)),   # 5 passes, LS later
    Case('unicycle', 'boxer', {}, {'ls_max': 2}, 2, 16, 1, 'cold', 0.0, 4, ('flag-8',)),   # 5 passes, LS later
    Case('arm', 'cfg4', {}, {'ls_max': 2}, 4, 16, 4, 'disturbed', 0.3, 14, ('flag-8',)),   # 5 passes, LS later
]
# (flag, iterations, passes) of the witness at the last step of the cases above, as the oracle gave them when found
EXPECT = {
    'arm-cfg4-acc_iters1-acc_obj_tol0.0001-s1-warm-w13': (2, 3, 4),
    'arm-cfg4-acc_iters3-max_iter20-s1-disturbed0.1-w8': (0, 20, 21),
    'arm-cfg4-ls_max2-s1-disturbed0.3-w0': (-8, 0, 4),
    'arm-chain6-tol_comp0.001-tol_eq1e-05-tol_ineq1e-05-tol_stat0.001-s2-disturbed0.3-w14': (1, 4, 5),
    'arm-chain4-acc_iters1-acc_obj_tol0.0001-s2-disturbed0.1-w0': (2, 3, 4),
    'arm-chain4-acc_iters3-max_iter20-s1-disturbed0.3-w8': (0, 20, 21),
    'arm-chain8-ls_max2-s2-disturbed0.3-w4': (-8, 0, 4),
    'arm-chain4-tol_comp0.001-tol_eq1e-05-tol_ineq1e-05-tol_stat0.001-s3-disturbed0.1-w0': (1, 4, 5),
    'chain3-wc_point-acc_iters1-acc_obj_tol0.0001-s1-disturbed0.1-w14': (2, 3, 4),
    'chain3-cfg2-acc_iters3-max_iter20-s4-cold-w8': (0, 20, 21),
    'chain3-cfg2-ls_max2-s1-disturbed0.1-w12': (-8, 0, 4),
    'chain3-wc_point-tol_comp0.001-tol_eq1e-05-tol_ineq1e-05-tol_stat0.001-s1-warm-w2': (1, 4, 5),
    'chain3-cfg2-t40-acc_iters1-acc_obj_tol0.0001-s2-disturbed0.1-w1': (2, 3, 4),
    'chain3-cfg2-t40-acc_iters3-max_iter20-s2-cold-w5': (0, 20, 21),
    'chain3-cfg2-t40-ls_max2-s1-disturbed0.1-w9': (-8, 0, 4),
    'chain3-cfg2-t40-tol_comp0.001-tol_eq1e-05-tol_ineq1e-05-tol_stat0.001-s3-warm-w14': (1, 5, 6),
    'point_slack-cfg2-sTrue-acc_iters1-acc_obj_tol0.0001-s4-warm-w8': (2, 3, 4),
    'point_slack-cfg2-sTrue-acc_iters3-max_iter20-s1-disturbed0.1-w10': (0, 20, 21),
    'point_slack-cfg2-sTrue-ls_max2-s1-cold-w14': (-8, 0, 4),
    'point_slack-cfg2-sTrue-tol_comp0.001-tol_eq1e-05-tol_ineq1e-05-tol_stat0.001-s2-disturbed0.1-w6': (1, 5, 6),
    'unicycle-cfg3-acc_iters1-acc_obj_tol0.0001-s1-warm-w1': (2, 3, 4),
    'unicycle-cfg3-acc_iters3-max_iter20-s3-cold-w5': (0, 20, 22),
    'unicycle-cfg3-ls_max2-s1-warm-w7': (-8, 0, 4),
    'unicycle-boxer-tol_comp0.001-tol_eq1e-05-tol_ineq1e-05-tol_stat0.001-s2-disturbed0.3-w2': (1, 3, 4),
    'chain3-wc_point-acc_iters1-acc_obj_tol0.0001-s2-cold-w7': (2, 8, 9),
    'point_slack-cfg2-sTrue-acc_iters1-acc_obj_tol0.0001-s1-cold-w0': (2, 11, 12),
    'arm-cfg4-acc_iters1-acc_obj_tol0.0001-s1-cold-w12': (2, 9, 10),
    'chain3-cfg2-t40-ls_max2-s2-disturbed0.3-w10': (-8, 1, 5),
    'point_slack-cfg2-sTrue-ls_max2-s3-disturbed0.1-w3': (-8, 1, 5),
    'unicycle-boxer-ls_max2-s2-cold-w4': (-8, 1, 5),
    'arm-cfg4-ls_max2-s4-disturbed0.3-w14': (-8, 1, 5),
}
# (class, branch): instances searched without a rounding-insensitive witness.  ('arm', 'flag2') stood here with 16320
# instances: true of acc_iters = 8 only, ACC reaches it in the first seed
UNREACHED = {
    ('point_slack', 'flag-7'): 3264,   # (never seen, rounding filter aside)
    ('unicycle', 'flag-7'): 13056,   # (never seen, rounding filter aside)
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


def oracle_loop(sc, o, c, inputs=None):
    """The closed loop on the oracle: a list with one entry per control step -- the inputs of the step (``x``, ``x0``,
    ``duals``: what each instance starts from) and ``cpu``, Oracle.solve_each of them.  The loop steps from the oracle's
    plan, so a device handle fed the same ``x`` / ``x0`` step by step solves the same problems.
    ``inputs``: another loop of the same scenario (an option variant of an edge case): its ``x`` / ``x0`` are solved
    step by step instead, under this oracle's options and from this loop's own multipliers -- what a handle created
    with those options and fed the same inputs does."""
    nxs, mu0 = o.nx + o.ns, sc.desc["options"]["mu0"]
    dist = disturbance(c, o.nx)
    x, x0 = sc.xinit.copy(), sc.x0.copy()
    duals = None
    out = []
    for t in range(c.steps):
        if inputs is not None:
            x, x0 = inputs[t]["x"], inputs[t]["x0"]
        cpu = o.solve_each(x, x0, sc.params, duals)
        out.append(dict(x=x.copy(), x0=x0.copy(), duals=duals, cpu=cpu))
        duals = [cpu["duals"][b] if cpu["exitflag"][b] >= 0 else failed_duals(o, mu0) for b in range(c.B)]
        if t + 1 < c.steps and inputs is None:
            z = cpu["z"]
            x = np.array([o.dynamics(x[b], z[b, 0, nxs:]) for b in range(c.B)]) + dist[t + 1]
            x0 = np.concatenate([z[:, 1:], z[:, -1:]], axis=1)
    return out


def is_loose(opts):
    return any(k.startswith("tol_") for k in opts)


def default_oracle(Oracle, sc, c):
    """The oracle of the case's scenario with the tolerances of LOOSE back at their defaults (everything else kept)."""
    return Oracle(dict(sc.desc, options=dict(sc.desc["options"], **{k: DEFAULT_TOL[k] for k in c.opts if k in DEFAULT_TOL})))


DEFAULT_TOL = {"tol_stat": 1e-6, "tol_eq": 1e-8, "tol_ineq": 1e-8, "tol_comp": 1e-6}     # (include/rmpc.h)


def census_view(o, sc, c, step, b, o_default=None):
    """What the predicates of BRANCHES look at: the census of instance b's solve at ``step``, its iteration count, and
    for a case under LOOSE the iterations the same inputs take at the default tolerances (``o_default``)."""
    cpu = step["cpu"]
    view = dict(cpu["census"][b], iters=int(cpu["iters"][b]))
    if o_default is not None and cpu["exitflag"][b] == 1:
        r = witness_solve(o_default, sc, c._replace(witness=b), step)
        view["default_iters"] = int(r["iters"]) if r["exitflag"] >= 1 else -1
    return view


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


# ---- edge witnesses: option variants of committed cases, derived by rule (derive_edges), not searched ----
# max_iter   a cold case whose witness ends with flag 1 (or 2) at iteration n: the same inputs under max_iter = n end
#            with that flag and n iterations -- converged and acceptable are tested before the iteration limit -- and
#            under max_iter = n - 1 with flag 0 and n - 1 iterations;
# acc_iters  a case whose witness ends with flag 2 under acc_iters = k: under acc_iters = 0 (off) it does not, and under
#            k + 1 it ends as the oracle says.
# A variant runs the case's loop on the case's inputs (oracle_loop's ``inputs``) under its own options from the first
# step on, as a handle created with them does.  Per class the first case in CASES all of whose variants finish within
# MAX_PASSES passes and pass the rounding filter.
# case: index into CASES; max_iter: (flag, n) of the exit; acc_iters: (2, k); expect: (flag, iterations, passes) of the
# witness at the last step under each variant, in edge_variants' order (pinned: the oracle's results when derived)
Edge = namedtuple("Edge", "kind case flag n expect")
EDGES = [
    Edge('max_iter', 10, 1, 19, ((1, 19, 20), (0, 18, 19))),
    Edge('max_iter', 50, 2, 8, ((2, 8, 9), (0, 7, 8))),
    Edge('acc_iters', 34, 2, 1, ((1, 4, 5), (1, 4, 5))),
    Edge('max_iter', 18, 1, 28, ((1, 28, 35), (0, 27, 34))),
    Edge('max_iter', 51, 2, 11, ((2, 11, 12), (0, 10, 11))),
    Edge('acc_iters', 19, 2, 8, ((1, 13, 14), (1, 13, 14))),
    Edge('max_iter', 21, 1, 13, ((1, 13, 17), (0, 12, 16))),
    Edge('max_iter', 24, 2, 18, ((2, 18, 37), (0, 17, 36))),
    Edge('acc_iters', 23, 2, 8, ((1, 11, 26), (1, 11, 26))),
    Edge('max_iter', 2, 1, 11, ((1, 11, 13), (0, 10, 12))),
    Edge('max_iter', 52, 2, 9, ((2, 9, 10), (0, 8, 9))),
    Edge('acc_iters', 26, 2, 1, ((1, 4, 5), (1, 4, 5))),
]
# (class, kind, flag) for which no committed case qualifies
EDGES_MISSING = {
}


def edge_id(e):
    return "%s%d-f%d-%s" % (e.kind, e.n, e.flag, case_id(CASES[e.case]))


def edge_variants(e):
    """[(label, option overrides)] of an edge."""
    if e.kind == "max_iter":
        return [("at", {"max_iter": e.n}), ("below", {"max_iter": e.n - 1})]
    return [("off", {"acc_iters": 0}), ("longer", {"acc_iters": e.n + 1})]


def _variant_loops(make_scenario, Oracle, c, base_loop, variants):
    out = []
    for label, over in variants:
        cv = c._replace(opts=dict(c.opts, **over))
        sc = scenario_of(make_scenario, cv)
        o = Oracle(sc.desc)
        out.append((label, cv, sc, o, oracle_loop(sc, o, cv, inputs=base_loop)))
    return out


@functools.lru_cache(maxsize=None)
def _edge_cached(make_scenario, Oracle, e):
    base = loop_of(make_scenario, Oracle, CASES[e.case])
    return base, _variant_loops(make_scenario, Oracle, CASES[e.case], base[2], edge_variants(e))


def edge_loops(make_scenario, Oracle, e):
    """((scenario, oracle, loop) of the edge's case, [(label, variant case, scenario, oracle, loop)]), once per session."""
    return _edge_cached(make_scenario, Oracle, e)


def result_of(cpu, b):
    return (int(cpu["exitflag"][b]), int(cpu["iters"][b]), int(cpu["passes"][b]))


def edge_holds(e, base_loop, variants):
    """The rule of an edge on the oracle's results (the witness at the last step)."""
    b = CASES[e.case].witness
    res = {label: (int(loop[-1]["cpu"]["exitflag"][b]), int(loop[-1]["cpu"]["iters"][b])) for label, _, _, _, loop in variants}
    cpu = base_loop[-1]["cpu"]
    if e.kind == "max_iter":
        return ((int(cpu["exitflag"][b]), int(cpu["iters"][b])) == (e.flag, e.n) and e.n >= 2
                and res["at"] == (e.flag, e.n) and res["below"] == (0, e.n - 1))
    return cpu["exitflag"][b] == 2 and CASES[e.case].opts.get("acc_iters", 8) == e.n and res["off"][0] != 2


def derive_edges(make_scenario, Oracle):
    """EDGES by the rule above, from CASES."""
    out = []
    for cls in CLASSES:
        for kind, flag in (("max_iter", 1), ("max_iter", 2), ("acc_iters", 2)):
            for i, c in enumerate(CASES):
                if c.cls != cls or (kind == "max_iter" and c.mode != "cold"):
                    continue
                sc, o, loop = loop_of(make_scenario, Oracle, c)
                cpu = loop[-1]["cpu"]
                if cpu["exitflag"][c.witness] != flag:
                    continue
                e = Edge(kind, i, flag, int(cpu["iters"][c.witness]) if kind == "max_iter" else c.opts.get("acc_iters", 8), ())
                if kind == "max_iter" and e.n < 2:
                    continue
                variants = _variant_loops(make_scenario, Oracle, c, loop, edge_variants(e))
                e = e._replace(expect=tuple(result_of(lp[-1]["cpu"], c.witness) for _, _, _, _, lp in variants))
                if edge_holds(e, loop, variants) and all(
                        lp[-1]["cpu"]["passes"][c.witness] <= MAX_PASSES and rounding_insensitive(ov, scv, cv, lp[-1])
                        for _, cv, scv, ov, lp in variants):
                    out.append(e)
                    break
    return out


# ---- the reported numbers (obj, kkt) where a test compares a witness with the oracle at flag 0, -8 or at a cut ----
OBJ_RTOL = 1e-9            # the bar of test_solve_matches_oracle
KKT_FLOOR = 1e-9           # points where the oracle's residual is below this are not compared
# Worst relative movement of the oracle's own residual max(res_stat, res_eq, res_ineq, res_comp), over all comparison
# points (comparison_points), under the rounding filter's eight draws of PERTURB_REL = 1e-8 on the inputs; measured and
# pinned by test_decision_census_cpu.py::test_kkt_rel_is_the_oracles_own_movement.  The input perturbation is about 1e5
# roundings; a stage missing from one of the maxima is O(1) away.
KKT_REL_MEASURED = 2.02e-4
KKT_REL = 8 * KKT_REL_MEASURED     # (the convention of exact_hessian_cases.REL)


def cut_iterations(c, first, iters):
    """Cold witnesses: the iterations one past the first firing of each of the case's branches, short of the last."""
    cuts = sorted({first[FIRST_OF.get(k, k)] + 1 for k in c.branches} - {0})
    return [f for f in cuts if f < iters]    # (at its last iteration the solve stops by itself)


def has_cuts(c):
    """Decidable without the oracle: a cold case with a branch that is not dated by the exit."""
    return c.mode == "cold" and any(FIRST_OF.get(k, k) != "exit" for k in c.branches)


def comparison_points(make_scenario, Oracle):
    """[(label, oracle, scenario, case, step)]: every solve at which test_gpu_decision_branches.py compares obj and kkt --
    the witness's solve at the LAST step (the one the rounding filter vouches for) where it ends with flag 0 or -8, cases
    and edge variants, and the cuts of the cold cases."""
    pts = []
    for c in CASES:
        sc, o, loop = loop_of(make_scenario, Oracle, c)
        if loop[-1]["cpu"]["exitflag"][c.witness] in (0, -8):
            pts.append(("%s step %d" % (case_id(c), len(loop) - 1), o, sc, c, loop[-1]))
        if has_cuts(c):
            b = c.witness
            for f in cut_iterations(c, loop[0]["cpu"]["first"][b], int(loop[0]["cpu"]["iters"][b])):
                oc = Oracle(dict(sc.desc, options=dict(sc.desc["options"], max_iter=f)))
                step = dict(x=sc.xinit, x0=sc.x0, duals=None)
                step["cpu"] = oc.solve_each(sc.xinit, sc.x0, sc.params)
                pts.append(("%s cut %d" % (case_id(c), f), oc, sc, c, step))
    for e in EDGES:
        _, variants = edge_loops(make_scenario, Oracle, e)
        for label, cv, scv, ov, lp in variants:
            if lp[-1]["cpu"]["exitflag"][cv.witness] in (0, -8):
                pts.append(("%s %s step %d" % (edge_id(e), label, len(lp) - 1), ov, scv, cv, lp[-1]))
    return pts


def kkt_of(r):
    return max(r["res_stat"], r["res_eq"], r["res_ineq"], r["res_comp"])


def kkt_movement(o, sc, c, step, draws=PERTURBATIONS):
    """(the oracle's residual at the point, its worst relative movement under the filter's draws)."""
    rng = np.random.default_rng(zlib.crc32(repr((c.name, c.seed, c.witness, "filter")).encode()))
    k0 = kkt_of(witness_solve(o, sc, c, step))
    return k0, max(abs(kkt_of(witness_solve(o, sc, c, step, rng)) - k0) for _ in range(draws)) / max(k0, 1e-300)
