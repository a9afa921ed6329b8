"""Inputs of tests/test_gpu_sweep_row_sums.py, shared with the recording of tests/golden/row_sums_parent.npz.

The sweep of the chain without slack keeps each row's share of the stage's partial results (sum of |g - t|, product
and exponent sum of the mantissas of t, the maxima and the sum of t * lambda, the positivity test) at the row under a
generated view.  The batches are the smallest that run the rows under every mask and regime; their seeds were chosen
by what the CPU oracle does on them (``Oracle.solve`` + ``orc_last_passes()``; a solve without a null pass or a
line-search retry needs iterations + 1 passes):

  b3    cfg2, B = 3, seed 409        oracle passes 16 / 22 / 12, iterations 15 / 19 / 11: instance 1 has two passes that
                                     are not fresh steps.  On the default grid the second wavefront has an idle half.  On
                                     one wavefront (RMPC_FUSED_GRID=1) the half of instance 0 finishes after 16 passes and
                                     takes instance 2 while its partner is at pass 17 of 22 (both copies of the sweep call
                                     in one pass, each under half a mask), and instance 2 ends alone at pass 28.
  n2    cfg2, horizon 2, seed 403    lanes k = 0 and k = N - 1 only: neutralised rows, no defect on the last stage
  n3    cfg2, horizon 3, seed 403    one inner stage; oracle passes 9 / 7 / 7
  cfg1  cfg1, B = 1                  the example model's view, half a wavefront
  warm  b3's batch, second solve     warm-started on the same handle from the oracle's first plan
  bad   b3's batch, damaged          instance 1 starts inside its first obstacle on every stage behind the pinned one (a
                                     non-positive row value under the inverse-barrier term), instance 2 has a NaN obstacle
                                     coordinate on stage 5 (non-finite row value): the oracle leaves both on their first
                                     pass with flag -7, instance 0 converges as in b3
"""
import numpy as np

KEYS = ("z", "exitflag", "iters", "kkt", "obj")

# key: (configuration, B, seed, scenario keywords, oracle's passes per instance)
BATCHES = {
    "b3": ("cfg2", 3, 409, {}, (16, 22, 12)),
    "n2": ("cfg2", 3, 403, {"time_horizon": 2}, (7, 7, 7)),
    "n3": ("cfg2", 3, 403, {"time_horizon": 3}, (9, 7, 7)),
    "cfg1": ("cfg1", 1, 0, {}, None),
}
BAD_FLAGS = (1, -7, -7)


def scenario(make_scenario, key):
    name, B, seed, kw, _ = BATCHES[key]
    return make_scenario(name, B=B, seed=seed, **kw)


def bad_inputs(sc):
    """(x0, params) of b3's batch with instances 1 and 2 damaged as the module text says"""
    d = sc.desc
    B, N, npar = sc.B, d["N"], d["npar"]
    P = np.array(sc.params, dtype=np.float64).reshape(B, N, npar).copy()
    x0 = np.array(sc.x0, dtype=np.float64).copy()
    c = P[1, 1, d["off_obst"]:d["off_obst"] + 2]
    x0[1, 1:, 0] = c[0]
    x0[1, 1:, 1] = c[1] + 0.05
    P[2, 5, d["off_obst"]] = np.nan
    return x0, P.reshape(np.shape(sc.params))


def oracle_warm_pair(Oracle, olib, sc):
    """b3's batch on the oracle, cold and then warm from its own plan and multipliers: per solve flags, iterations,
    passes and plans"""
    o = Oracle(sc.desc)
    out = []
    duals, x0 = [None] * sc.B, sc.x0
    for _ in range(2):
        z = np.zeros((sc.B, o.N, o.nv))
        flag, iters, passes = (np.zeros(sc.B, dtype=np.int32) for _ in range(3))
        for b in range(sc.B):
            r = o.solve_warm(sc.xinit[b], x0[b], sc.params[b], duals[b])
            z[b], flag[b], iters[b], passes[b], duals[b] = r["z"], r["exitflag"], r["iters"], olib().orc_last_passes(), r["duals"]
        out.append(dict(z=z, exitflag=flag, iters=iters, passes=passes))
        x0 = z
    return out


def solve_all(Solver, sc_of, warm_x0):
    """Every batch on a handle of its own, as the environment selects the path: {key: result + last_passes}.
    sc_of(key): the scenario; warm_x0: the oracle's first plan of b3 (the warm solve's initial guess)."""
    out = {}
    for key in BATCHES:
        sc = sc_of(key)
        s = Solver(sc.desc, max_batch=sc.B)
        assert s.is_fused()
        r = s.solve(sc.xinit, sc.x0, sc.params)
        out[key] = dict(r, last_passes=s.last_passes())
        if key == "b3":
            x0, P = bad_inputs(sc)
            r = s.solve(sc.xinit, x0, P)   # (same handle: a failed solve leaves nothing behind that the next one reads)
            out["bad"] = dict(r, last_passes=s.last_passes())
            s.close()
            s = Solver(sc.desc, max_batch=sc.B)
            s.set_warm_start(True)
            s.solve(sc.xinit, sc.x0, sc.params)
            r = s.solve(sc.xinit, warm_x0, sc.params)
            out["warm"] = dict(r, last_passes=s.last_passes())
        s.close()
    return out


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
