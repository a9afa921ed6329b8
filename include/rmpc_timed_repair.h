/* rmpc_timed_repair.h -- timed routes whose failing priority orders are repaired on the device:
 * failure-driven re-prioritisation (Bennewitz, Burgard, Thrun 2002; the restart rule of priority-based search) around
 * the plan of rmpc_timed_plan_device.  A header of its own beside rmpc.h, whose entries are what they were and whose
 * words -- cell, CONFLICT, res, rules 1 to 8, status, arrive, key, best -- are used here as they stand there.  Written in
 * the forms robot_mpcs_amd/_abi.py reads.
 *
 * rmpc_timed_plan_repair_device takes what rmpc_timed_plan_device takes (the members of rmpc_timed_repair up to `best`
 * are those of rmpc_timed_plan, in its order and with its meaning) and a number of repair rounds R = rounds.  For every
 * row g of orders, on its own:
 *  1. o_0 is the caller's row.  A row that is no permutation is reported as rmpc_timed_plan_device reports it
 *     (RMPC_TIMED_BAD_ORDER, paths -1, arrive T + 1, key INT64_MAX); its order_out is all -1, its rounds_run 0 and its
 *     round_best -1.
 *  2. Round r = 0, 1, ... is o_r planned by rules 1 to 8 of rmpc_timed_plan_device as they stand, from an empty res and
 *     the later-ranked starts of o_r; its key is k_r.
 *  3. A robot is BAD in round r when its status > 0, or its status == 0 and its arrive > T.  A skipped robot
 *     (RMPC_GRID_OUTSIDE) is never bad.
 *  4. The search stops behind round r when no robot is bad, or r == R, or o_{r+1} == o_r; otherwise it goes on with
 *     o_{r+1} = the bad robots of round r in their rank order of o_r, then all the others in their rank order of o_r (a
 *     stable partition: who could not be planned behind the others is planned ahead of them).
 *  5. paths, status, arrive, key and order_out of the row are those of the round with the least (k_r, r); round_best [g]
 *     is that r, rounds_run [g] the number of rounds planned (1 .. R + 1).
 *  6. best is the g with the least (key, g) among the rows that are permutations, -1 without one.
 * It follows that with R = 0 every output is that of rmpc_timed_plan_device and order_out the input; that the outputs of
 * row g are what rmpc_timed_plan_device gives on order_out [g], so its GUARANTEE and rmpc_timed_follow_device carry over
 * unchanged; and that key [g] is never above the key of round 0.  Everything is integer work on cells except the ranking
 * of end cells: every result is bitwise the same on every run.
 *
 * One workgroup per row; no host reads, no synchronisation, takes a stream, runs on the device of grid.
 * work: rmpc_timed_plan_repair_work_bytes(H, W, T, G, B) bytes (-1 for sizes that are refused), contents irrelevant.
 * Refused before any HIP call (-1, rmpc_last_error): what rmpc_timed_plan_device refuses, a struct_size other than
 * sizeof(rmpc_timed_repair), rounds outside [0, RMPC_TIMED_MAX_ROUNDS], NULL order_out, rounds_run or round_best, a
 * workspace that is too small. */
#ifndef RMPC_TIMED_REPAIR_H
#define RMPC_TIMED_REPAIR_H

#include <stdint.h>

#include "rmpc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RMPC_TIMED_MAX_ROUNDS 16

typedef struct rmpc_timed_repair {
  int32_t struct_size;                 /* sizeof(rmpc_timed_repair) */
  int32_t H, W, movement;
  const double *grid;                  /* [H][W] */
  double occ_threshold;
  int32_t B, Gf;
  const int32_t *start_cell;           /* [B] */
  const int32_t *goal_index;           /* [B] into fields / goal_cells */
  const double *fields;                /* [Gf][H][W] */
  const int32_t *goal_cells;           /* [Gf] */
  int32_t T, sep2, lag, G;
  const int32_t *orders;               /* [G][B] */
  void *work; int64_t work_bytes;      /* rmpc_timed_plan_repair_work_bytes(H, W, T, G, B) */
  int32_t *paths, *status, *arrive;    /* [G][B][T + 1], [G][B], [G][B] out */
  int64_t *key;                        /* [G] out */
  int32_t *best;                       /* one int32 out */
  int32_t rounds;                      /* R: repair rounds behind round 0 */
  int32_t *order_out;                  /* [G][B] out: the order whose plan the row reports */
  int32_t *rounds_run, *round_best;    /* [G], [G] out */
} rmpc_timed_repair;

int64_t rmpc_timed_plan_repair_work_bytes(int H, int W, int T, int G, int B);
int rmpc_timed_plan_repair_device(const rmpc_timed_repair *p, void *stream);

#ifdef __cplusplus
}
#endif

#endif
