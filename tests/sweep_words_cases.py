"""Inputs of tests/test_gpu_sweep_words.py, shared with the recording of tests/golden/sweep_words_parent.npz.

The merged sweep call of the point robot's fused kernel no longer stores or reads the values of the twelve general
single-variable rows (the limits of q and u): it forms them from the iterate and the limit, and asks for the operands
of the step lengths first (SWEEPWORDS, rmpc_sweep.hpp).  The batches are those of tests/sweep_row_sums_cases.py -- b3
(seed 409: instance 1 has two passes that are not fresh steps, so that the current buffer's row values are those of
an older sweep), n2 / n3 (the pinned stage's general rows, the clamp of the last stage), cfg1 (the other view), b3's
warm second solve and its damaged copy; that file says how their seeds were chosen -- and one more:

  lim   cfg2, B = 3, seed 409, the limit words of every stage's parameter row (13 .. 24: lower / upper limits of q,
        lower / upper limits of u) scaled by a factor of their own, drawn from [0.75, 1.25] (generator seeded with
        LIM_SEED) per instance, stage and word: a limit taken from another stage, instance or row changes the value
        of a row, and with it bytes of the plan.  Chosen with the CPU oracle (``Oracle.solve`` + ``orc_last_passes()``)
        as the first of the seeds 1, 2, ... on which every instance converges with a thrust limit active somewhere in
        the plan (|u| within 1e-3 of its scaled bound on some stage) -- the rows do shape the result: oracle passes
        LIM_PASSES.
"""
import copy

import numpy as np

import sweep_row_sums_cases as rs
from sweep_row_sums_cases import BAD_FLAGS, KEYS, bad_inputs, oracle_warm_pair, same_bytes  # noqa: F401

LIM_SEED = 1
LIM_WORDS = (13, 25)   # the general rows' limits in a stage's parameter row (v_poff of the generated view)
LIM_PASSES = (13, 23, 12)   # iterations 12 / 20 / 11
# key: (configuration, B, seed, scenario keywords, oracle's passes per instance)
BATCHES = dict(rs.BATCHES, lim=("cfg2", 3, 409, {}, LIM_PASSES))


def lim_params(sc, seed=LIM_SEED):
    """the batch's parameters with every limit word scaled on its own"""
    d = sc.desc
    P = np.array(sc.params, dtype=np.float64).reshape(sc.B, d["N"], d["npar"]).copy()
    f = np.random.default_rng(seed).uniform(0.75, 1.25, size=(sc.B, d["N"], LIM_WORDS[1] - LIM_WORDS[0]))
    P[:, :, LIM_WORDS[0]:LIM_WORDS[1]] *= f
    return P.reshape(np.shape(sc.params))


def scenario(make_scenario, key):
    name, B, seed, kw, _ = BATCHES[key]
    sc = make_scenario(name, B=B, seed=seed, **kw)
    if key == "lim":
        sc = copy.copy(sc)
        sc.params = lim_params(sc)
    return sc


def solve_all(Solver, sc_of, warm_x0):
    """Every batch on a handle of its own, as the environment selects the path: {key: result + last_passes}.
    sc_of(key): the scenario; warm_x0: the oracle's first plan of b3 (the warm solve's initial guess)."""
    out = rs.solve_all(Solver, sc_of, warm_x0)
    sc = sc_of("lim")
    s = Solver(sc.desc, max_batch=sc.B)
    assert s.is_fused()
    out["lim"] = dict(s.solve(sc.xinit, sc.x0, sc.params), last_passes=s.last_passes())
    s.close()
    return out
