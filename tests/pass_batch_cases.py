"""Cases shared by the tests of the pass kernels' batch machinery (test_gpu_pass_batch.py, the migration tests of
test_gpu_parity.py, the pass-kernel cases of test_gpu_warm_start.py): the host loop of solve_device switches regime by
size, and every case here sits at one of the switches.  Each test asserts through ``Solver.last_solve_path()``
(rmpc_last_solve_path) that its solve ran in the regime it names.

  list >= kGroupedMin = 512      k_riccati's grouped blocks (models with at most 8 states: Cfg::IPB = 4), handed over to
                                 the one-wave blocks once the list -- the whole batch while more than an eighth of it
                                 iterates, the instances still iterating afterwards -- is shorter
  B >= kMigrateMin = 1024        the survivors move to the compact workspace (k_migrate) at the first look of the host
                                 loop (after 8, 10, 12, ... passes) that finds at most B / kDenseDiv = B / 8 iterating
  B > kCompactWaveMax = 8192     k_compact (one block of 1024 threads) builds the list instead of k_compact_wave
  B >= kLaneMin = 16384          k_riccati_lane for the chains with at most 3 joints, until the migration

Batch sizes are deliberately no multiples of 64 or of a block's instance count (8 in the grouped blocks of the small
models, 4 otherwise).

Seeds of the migration cases.  Whether a batch migrates, and how many instances move, follows from how many passes
(horizon evaluations) each instance needs; the oracle counts them (orc_last_passes).  An instance still iterates after
P passes when it needs more than P.  The seeds below are those for which the oracle's counts OVER THE WHOLE BATCH
predict a migration of at least 8 survivors; the prediction is a way to choose inputs, what the tests assert is the
query.  Oracle, instances iterating after the looks around the migration:

  cfg2   B 2048 seed 7        look 14: 485 (23.7 %)   look 16: 128 (6.3 %)  -> 128 move after 16 passes
  cfg3   B 1280 seed 8        look 26: 162 (12.7 %)   look 28: 125 (9.8 %)  -> 125 move after 28 passes
  cfg4   B 1024 seed 9        look 12: 437 (42.7 %)   look 14:  25 (2.4 %)  ->  25 move after 14 passes
  chain4 B 1024 seed 10 N 24   look 12: 479 (46.8 %)   look 14:  43 (4.2 %)  ->  43 move after 14 passes
      (at their own horizon of 16 stages chain4 and chain8 finish too much alike for a batch of 1024: seeds 10 .. 30 of
       chain4 leave 130 .. 165 iterating after 12 passes, just over an eighth, and 0 or 1 after 14; chain8, seed 10, 299
       and 3.  With 24 stages the counts spread.)
  cfg2   B 1536 seed 11 N 40   look 16: 355 (23.1 %)   look 18: 181 (11.8 %) -> 181 move after 18 passes
      (181 against a bar of 192: should a few instances of the device take two passes longer, 88 move after 20)
  cfg2   B 1024 seed 7        look 14: 258 (25.2 %)   look 16:  78 (7.6 %)  ->  78 move after 16 passes
      (the cold first step of test_gpu_warm_start.py::test_warm_loop_across_a_migration)

The stall counter of the acceptable stop across a migration (STALL_MIGRATION below).  In a cold batch the feasible,
stagnant end game comes long after the migration: over cfg2 B 1024 and cfg3 B 1280, seeds 7 .. 12, windows of 3, 5 and
8 at acc_obj_tol 1e-4 and 1e-3, every survivor that ends with flag 2 begins its last stagnant run 17 passes or more after
the move, and the survivors that are stagnant at the move converge one pass later, where the converged test comes
before the counter is read.  In the WARM second step the batch is feasible from the start and migrates at the first
look, after 8 passes:
  cfg3   B 1280 seed 10, acc_iters 3, acc_obj_tol 1e-4, step 1   look 8: 87   -> 87 move after 8 passes; 19 of them
      end with flag 2, and for at least six (181, 571, 780, 912, 919, 1273) the run of three stagnant iterations that
      ends the solve began at iteration 4, evaluated by pass 7: the counter crosses k_migrate at 1 or more and is what
      decides the flag-2 exit at iteration 6.  (decision_cases.ACC itself, acc_iters = 1, cannot show this: the first
      stagnant iteration ends the solve.)
"""
import numpy as np

NO_FUSED = {"RMPC_NO_FUSED": "1"}

# (name, B, seed, make_scenario overrides, environment at rmpc_create)
MIGRATION_CASES = [
    ("cfg2", 2048, 7, {}, NO_FUSED),
    ("cfg3", 1280, 8, {}, NO_FUSED),
    # ric_arm_block inside k_riccati: LDS image slots, one instance per block
    ("cfg4", 1024, 9, {}, NO_FUSED),
    # ric_backward, the dense path (on the pass kernels by itself: no fused kernel for 4 or 8 joints)
    ("chain4", 1024, 10, {"time_horizon": 24}, {}),
    # a horizon beyond the fused kernel's 32 stages: the production route to these kernels, no switch
    ("cfg2", 1536, 11, {"time_horizon": 40}, {}),
]


# (name, B, seed, option overrides, environment at rmpc_create): see above
STALL_MIGRATION = ("cfg3", 1280, 10, {"acc_iters": 3, "acc_obj_tol": 1e-4}, NO_FUSED)


def carried_stall_decides(o, desc, x, x0, params, duals, migrated_at):
    """Oracle census of one instance of a batch that migrated after ``migrated_at`` passes: True when the instance is a
    survivor (needs more passes), ends with flag 2, and the unbroken run of acc_iters stagnant iterations that ends it
    began at an iteration evaluated within those passes -- so the counter is non-zero when the survivors move, is not
    reset afterwards, and its carried value decides the exit.  (The passes an instance has used when it reaches
    iteration i are those of its solve under max_iter = i.)  Returns (verdict, the oracle's result)."""
    k = desc["options"]["acc_iters"]
    r = o.solve_warm(x, x0, params, duals)
    if r["exitflag"] != 2 or r["passes"] <= migrated_at:
        return False, r
    began = r["iters"] - k + 1      # (stall >= k at the exit: the last k iterations were stagnant in a row)
    cut = type(o)(dict(desc, options=dict(desc["options"], max_iter=began))).solve_warm(x, x0, params, duals)
    return bool(cut["exitflag"] == 0 and cut["iters"] == began and cut["passes"] <= migrated_at), r


def case_id(case):
    name, B, seed, kw = case[:4]
    return "-".join([name, str(B), str(seed)] + ["%s%s" % (k[0].upper(), v) for k, v in sorted(kw.items())])


# Grouped regime and its hand-over: (name, B, seed, make_scenario overrides, recursion kernel of the first pass).  Below
# kMigrateMin the host loop looks after 8, 12, 16, ... passes; the hand-over is on record once a look finds at most B / 8
# instances iterating (the list is the whole batch until then) and at least one.  Oracle, instances iterating:
#   cfg2   B 577 seed 51        look 12: 383   look 16: 42   look 20: 14   look 24: 3   (44 passes at the most)
#   cfg3   B 577 seed 52        look 24: 84    look 32: 25                              (123 passes at the most)
#   chain4 B 530 seed 54 N 32   look 12: 408   look 16: 18   look 20: 3                 (22 passes at the most; at its own 16
#                                                            stages nothing is left at look 16 and the host never sees the hand-over)
#   cfg4   B 530 seed 53        look 12: 234   look 16: 2                               (19 passes at the most)
# The arms with more than 4 joints (more than 8 states) have no grouped blocks (Cfg::IPB = 1, rmpc_model.hpp: "the arm
# runs one-wavefront blocks only"): cfg4 at 530 launches k_riccati<C, 1> on 530 blocks from the first pass on, and that
# is what its case asserts.
GROUPED_CASES = [
    ("cfg2", 577, 51, {}, "grouped"),
    ("cfg3", 577, 52, {}, "grouped"),
    ("cfg4", 530, 53, {}, "wave"),
    ("chain4", 530, 54, {"time_horizon": 32}, "grouped"),
]

# Sizes past kCompactWaveMax and kLaneMin; the chunks are solved through a handle below both
B_COMPACT_BLOCK = 8192 + 65
B_LANE = 16384 + 37
CHUNK = 2048
ORACLE_SAMPLE = 1024      # instances of a large batch the oracle solves (strided over the batch; no fewer)


def strided_sample(B, count):
    """count indices spread evenly over 0 .. B - 1, first and last column included."""
    idx = np.unique(np.round(np.linspace(0, B - 1, count)).astype(np.int64))
    assert len(idx) == count and idx[0] == 0 and idx[-1] == B - 1
    return idx


def take(res, idx):
    """The instances idx of a result dict (instances are independent: slices of the outputs are results)."""
    return {k: v[idx] for k, v in res.items()}


def solve_in_chunks(solver, xinit, x0, params, chunk):
    """The batch chunk by chunk through one handle: the joined results and each chunk's ``last_solve_path()``."""
    parts, paths = [], []
    for c in range(0, xinit.shape[0], chunk):
        parts.append(solver.solve(xinit[c:c + chunk], x0[c:c + chunk], params[c:c + chunk]))
        paths.append(solver.last_solve_path())
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}, paths
