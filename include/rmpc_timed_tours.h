/* rmpc_timed_tours.h -- timed tours: conflict-free space-time routes through every robot's stops, and the follower that
 * keeps their order and serves a stop only when the robot is on it.  A header of its own beside rmpc.h
 * and rmpc_tours.h: their entries are what they were.  Written in the forms robot_mpcs_amd/_abi.py reads.
 *
 * rmpc_timed_tours_plan_device is rmpc_timed_plan_device (rmpc.h, whose words -- cell, d2, CONFLICT, res, reach, the
 * moves, rules 1 to 8 -- are used here as they stand there) with a tour in place of the one goal: robot b visits the
 * cells goal_cells [stops [b][0 .. len [b] - 1]] in this order, stands `dwell` further layers on each, and then parks by
 * the field park_index [b].  The last stop's index there gives an open tour, a depot's or the start's field a return
 * leg.  Everything is integer work on cells except the ranking of end cells, which compares the doubles of a field as
 * written: every result is bitwise the same on every run.
 *
 * The rule for order g.  Robots are taken in rank order; res, the later-ranked starts, the free cells, the moves, the
 * start's exemption, stamping (rule 8) and the row that is no permutation are exactly those of rmpc_timed_plan_device.
 *  1. robot b is SKIPPED when start_cell [b] lies outside [0, H W), len [b] outside [0, K], any of its first len [b]
 *     stops outside [0, Gf), or park_index [b] outside [0, Gf): status RMPC_GRID_OUTSIDE, path all -1, arrive T + 1,
 *     served 0, serve_at all -1; its len [b] stops (0 when len [b] is out of range) count as unserved; it stamps nothing
 *     and blocks nobody.
 *  2. The state is t0 = 0, at = the start.  For leg j = 0 .. len [b] - 1 with the stop cell s = goal_cells [stops [b][j]]:
 *     reach[t0] = {at} (exempt from every test, as the start is), and reach[t], t = t0 + 1 .., by rule 3 of the timed
 *     plan (`t <= lag` counts layers from 0, not from t0).  The stop is SERVED at the least a >= t0 with
 *       - reach[a] holds s (a = t0 is tested before the first layer is swept: a robot that stands on its stop is served
 *         there; an s outside the map is in no layer),
 *       - a + dwell <= T,
 *       - s is HELD: for every u in a + 1 .. a + dwell, res[u] does not hold s, and for u <= lag s does not conflict
 *         with the start of a later-ranked robot that is not skipped.
 *     Then p[a .. a + dwell] = s, the leg is backtracked from (a, s) down to t0 by rule 6 (wait first, else the first
 *     move in move order), serve_at [b][j] = a, and the next leg starts from t0 = a + dwell, at = s.
 *  3. The leg FAILS when a layer f > t0 comes up empty before such an a, or there is no such a up to T.  In the first
 *     case te = f - 1 and status = f, in the second te = T and status = 0.  The end cell is the least (D(c), c) of
 *     reach[te] with D = fields [stops [b][j]] (rule 5); p[te .. T] = the end cell, backtracked down to t0; the
 *     len [b] - j stops from j on are unserved (serve_at -1); arrive = T + 1.  No parking leg follows.
 *  4. With every stop served the PARKING LEG runs rules 3 to 7 of the timed plan from (t0, at) with
 *     D = fields [park_index [b]]: reach[t0] = {at}, layers t0 + 1 .. T, status = f, te, the end cell, p[te .. T], the
 *     backtrack down to t0; arrive = the least a >= t0 with p[a .. T] all equal to goal_cells [park_index [b]], T + 1
 *     when there is none.
 *  5. The robot stamps its path (rule 8; a failed one too) and adds to fails (status > 0), late (arrive > T, skipped
 *     robots too), sum_arrive and unserved.
 * Outputs: paths, status, arrive, key as in the timed plan (key = (fails << 44) | (late << 32) | sum_arrive);
 * serve_at [G][B][K] int32: the layer stop j is reached, -1 when it is unserved or j >= len; served [G][B] int32: the
 * stops served; unserved [G] int32: the sum over the robots of len - served; best: one int32, the g with the least
 * (unserved, key, g) among the rows that are permutations, -1 when there is none.  A row that is not a permutation gets
 * what the timed plan gives it (RMPC_TIMED_BAD_ORDER, paths -1, arrive T + 1, key INT64_MAX) and serve_at -1, served 0,
 * unserved INT32_MAX.
 *
 * CONSEQUENCES.
 *  - With every len [b] = 0 and park_index = goal_index, paths, status, arrive, key and best equal those of
 *    rmpc_timed_plan_device bit for bit (rule 4 from (0, start) is its rules 2 to 7; unserved is 0 in every valid row).
 *  - The GUARANTEE of the timed plan carries over: between two robots i, j of one order that both have status 0,
 *    d2(p_i[t], p_j[s]) >= sep2 whenever |s - t| <= lag.  Every p[t], t >= 1, of the later-ranked one was admitted
 *    through res[t]: the cells of a leg because they lie in reach[t], the dwell cells a + 1 .. a + dwell by the held
 *    test, which asks of s what rule 3 asks of a cell; p[a] itself lies in reach[a] (or is the start at a = 0).
 *  - serve_at [b][0 .. served - 1] ascends with gaps of at least dwell, and p[a .. a + dwell] is the stop's cell for
 *    every a in it.
 *  - A robot's whole tour sweeps at most T layers: leg j sweeps t0 + 1 .. a and the next one starts at a + dwell >= a.
 * LIMIT, not fixed here: the rule is greedy per leg -- the earliest service.  It is no search over the product of cell
 * and leg, so an early service can strand a robot in a pocket that a later one would have avoided.  The G orders are
 * the remedy, as for the timed plan.
 *
 * work: rmpc_timed_tours_work_bytes(H, W, T, G) bytes, the same as rmpc_timed_plan_work_bytes: the history is reused
 * leg by leg.  Contents irrelevant.  Needs no handle; every pointer is a device pointer; the call runs on the device of
 * grid, takes a stream, allocates nothing and never synchronises.
 * Refused before any HIP call (-1, rmpc_last_error): what rmpc_timed_plan_device refuses, a struct_size other than
 * sizeof(rmpc_timed_tours), a NULL stops, len, park_index, serve_at, served or unserved, K outside
 * [1, RMPC_TIMED_TOURS_MAX_STOPS], dwell outside [0, RMPC_TIMED_TOURS_MAX_DWELL], G B K beyond INT_MAX.
 *
 * rmpc_timed_tours_follow_device is rmpc_timed_follow_device (rmpc.h) with stops; its rule stands at the declaration. */
#ifndef RMPC_TIMED_TOURS_H
#define RMPC_TIMED_TOURS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMPC_TIMED_TOURS_MAX_STOPS 64
#define RMPC_TIMED_TOURS_MAX_DWELL 64

typedef struct rmpc_timed_tours {
  int32_t struct_size;                 /* sizeof(rmpc_timed_tours) */
  int32_t H, W, movement;
  const double *grid;                  /* [H][W] */
  double occ_threshold;
  int32_t B, Gf;
  const int32_t *start_cell;           /* [B] */
  int32_t K, dwell;                    /* the most stops per robot; layers a robot stands on a stop after reaching it */
  const int32_t *stops;                /* [B][K] into fields / goal_cells; entries past len [b] are not read */
  const int32_t *len;                  /* [B] */
  const int32_t *park_index;           /* [B] into fields / goal_cells */
  const double *fields;                /* [Gf][H][W] */
  const int32_t *goal_cells;           /* [Gf] */
  int32_t T, sep2, lag, G;
  const int32_t *orders;               /* [G][B] */
  void *work; int64_t work_bytes;
  int32_t *paths, *status, *arrive;    /* [G][B][T + 1], [G][B], [G][B] out */
  int64_t *key;                        /* [G] out */
  int32_t *best;                       /* one int32 out */
  int32_t *serve_at, *served;          /* [G][B][K], [G][B] out */
  int32_t *unserved;                   /* [G] out */
} rmpc_timed_tours;

int64_t rmpc_timed_tours_work_bytes(int H, int W, int T, int G);
int rmpc_timed_tours_plan_device(const rmpc_timed_tours *p, void *stream);

/* rmpc_timed_follow_device with stops: one simultaneous step of all B robots along one order's d_paths [B][T + 1].
 * d_serve_at [B][K] int32: that order's serve_at; d_leg [B] int32, in and out: the stops served so far; d_served [B][K]
 * int32: entry (b, leg) is written once, with `now`, when that stop is served.  Per robot b whose path is valid, with
 * i = d_idx_in [b] clamped to [0, T], leg = d_leg [b] (at least 0) and dist the distance from d_pos [b * stride + 0 .. 1]
 * to the centre of p_b[i]:
 *  - when leg < K, d_serve_at [b][leg] == i and dist <= stop_tol: d_served [b][leg] = now and leg += 1.  At most one
 *    serve per call.
 *  - the robot then advances to i + 1 under the two tests of rmpc_timed_follow_device, with two changes: stop_tol takes
 *    the place of threshold when i equals any of d_serve_at [b][0 .. K - 1], and there is no advance while a stop at i is
 *    still pending (after the serve above: leg < K and d_serve_at [b][leg] == i).
 * One advance per call, so `dwell` layers cost at least `dwell` control steps.  d_idx_out (another buffer than d_idx_in),
 * d_blocked (may be NULL; -1 also while a stop is pending), d_goal and the robot whose path starts with -1 (it keeps
 * index, leg and goal, and blocks nobody) are as in rmpc_timed_follow_device.  With every d_serve_at = -1 the call
 * equals rmpc_timed_follow_device bit for bit and leaves d_leg and d_served as they are.  LIVENESS is that of
 * rmpc_timed_follow_device: the robot whose pending layer is least is not blocked, and a pending stop ends as soon as
 * the robot is within stop_tol of the cell it is sent to.
 * Refused before any HIP call: what rmpc_timed_follow_device refuses, a NULL d_serve_at, d_leg or d_served, K outside
 * [1, RMPC_TIMED_TOURS_MAX_STOPS], a stop_tol that is negative or NaN. */
int rmpc_timed_tours_follow_device(int B, int T, const int32_t *d_paths, const int32_t *d_idx_in, int32_t *d_idx_out,
                                   const double *d_pos, int stride, int W, double x0, double y0, double cell,
                                   double threshold, int sep2, int lag, double *d_goal, int32_t *d_blocked, int K,
                                   const int32_t *d_serve_at, int32_t *d_leg, int32_t *d_served, int now, double stop_tol,
                                   void *stream);

#ifdef __cplusplus
}
#endif

#endif
