/* rmpc_timed_replan.h -- lifelong timed tours: re-plan part of a fleet inside the layer frame of the plan it follows,
 * around routes that are reserved.  A header of its own beside rmpc.h and rmpc_timed_tours.h, whose
 * entries are what they were and whose words -- cell, d2, CONFLICT, res, reach, the moves, rules 1 to 8, legs, held --
 * are used here as they stand there.  Written in the forms robot_mpcs_amd/_abi.py reads.
 *
 * THE RESERVATION TABLE.  T + 1 layers of L = H Wd 64-bit words, Wd = ceil(W / 64): cell (row, col) of layer t is bit
 * col & 63 of word t L + row Wd + col / 64.  Bits past column W - 1 are never set.  rmpc_timed_reserve_words(H, W, T) is
 * its size in words (host only; -1 on sizes that are refused).
 *
 * rmpc_timed_reserve_device is rule 8 for given paths: for every row p with d_use == NULL or d_use [p] != 0 and every
 * t, with c = d_cells [p][t]: when c lies in [0, H W), the cells with d2 < sep2 of c are set in layer s for every s in
 * [0, T] with |s - t| <= lag; a c outside the map stamps nothing at that layer.  clear != 0 empties the table first,
 * clear == 0 ORs into what is there (a second call can add paths with another sep2).  One workgroup per row.  Limits: P
 * in [1, RMPC_TIMED_RESERVE_MAX_PATHS]; H W, T, sep2 and lag within the timed plan's limits.  It allocates nothing,
 * takes a stream, never synchronises, and runs on the device of d_res.
 *
 * rmpc_timed_tours_replan_device is rmpc_timed_tours_plan_device with these changes, and no others:
 *  1. In every order res[t] starts as layer t of res0 (empty when res0 is NULL) instead of empty.
 *  2. A robot with active [b] == 0 is KEPT: status RMPC_TIMED_KEPT, path all -1, arrive 0, served 0, serve_at all -1.  It
 *     is not planned, stamps nothing, is in no mask, and adds nothing to fails, late, sum_arrive or unserved.  Its route
 *     is expected to be in res0.  It still has its place in the permutation.
 *  3. An active robot is also SKIPPED (rule 1) when begin [b] lies outside [0, T].  Otherwise its state starts at
 *     t0 = begin [b], at = start_cell [b], and p[0 .. begin [b]] = start_cell [b]: the robot stands where it stands until
 *     its layer.  Layers, serve_at, a positive status and arrive are absolute.
 *  4. THE STANDING RULE takes the place of "for t <= lag, c does not conflict with the start of a later-ranked robot
 *     that is not skipped": c does not conflict with the start of any OTHER active robot r that is not skipped while
 *     t <= begin [r] + lag, whatever r's rank.  The held test changes in the same way: u <= begin [r] + lag.  (An
 *     earlier-ranked r has stamped its start's disc into res[0 .. begin [r] + lag] already, so with every begin 0 the
 *     rule admits exactly what the old one admits.)
 *  5. clash [b] = 1 when b is active, not skipped, and layer begin [b] of res0 holds start_cell [b] -- something reserved
 *     within lag layers of where the robot stands conflicts with it -- else 0.  It does not depend on the order.
 * key, unserved and best are as in the timed tours.
 *
 * GUARANTEE.  Let i be an active robot with status 0 and t > begin [i].  Then d2(p_i[t], q[s]) >= sep2 whenever
 * |s - t| <= lag, for q any path stamped into res0, the whole path (standing layers included) of any earlier-ranked
 * active robot of the same order, and the standing layers s <= begin [j] of any other active robot j.  Starts of two
 * active robots closer than sep2 are the caller's choice, as before.
 *
 * work: rmpc_timed_replan_work_bytes(H, W, T, G) bytes, contents irrelevant; p->work and p->work_bytes are not read.
 * Refused before any HIP call (-1, rmpc_last_error): what rmpc_timed_tours_plan_device refuses (but for its work), a
 * struct_size other than sizeof(rmpc_timed_replan), a NULL or too small work.  Everything else is decided on the
 * device. */
#ifndef RMPC_TIMED_REPLAN_H
#define RMPC_TIMED_REPLAN_H

#include <stdint.h>

#include "rmpc_timed_tours.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RMPC_TIMED_RESERVE_MAX_PATHS 4096
#define RMPC_TIMED_KEPT (-9)            /* the status of a robot that was not re-planned */

typedef struct rmpc_timed_replan {
  int32_t struct_size;                 /* sizeof(rmpc_timed_replan) */
  const uint64_t *res0;                /* the reservation table, or NULL = empty */
  const int32_t *active;               /* [B]; NULL = all active */
  const int32_t *begin;                /* [B]; NULL = all 0 */
  int32_t *clash;                      /* [B] out; may be NULL */
  void *work; int64_t work_bytes;      /* rmpc_timed_replan_work_bytes(H, W, T, G) */
} rmpc_timed_replan;

int64_t rmpc_timed_reserve_words(int H, int W, int T);
int rmpc_timed_reserve_device(int H, int W, int T, int P, const int32_t *d_cells, const int32_t *d_use, int sep2, int lag,
                              int clear, uint64_t *d_res, void *stream);
int64_t rmpc_timed_replan_work_bytes(int H, int W, int T, int G);
int rmpc_timed_tours_replan_device(const rmpc_timed_tours *p, const rmpc_timed_replan *x, void *stream);

#ifdef __cplusplus
}
#endif

#endif
