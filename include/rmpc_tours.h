/* rmpc_tours.h -- tours of several tasks per robot on the device, and a follower that stops at them, a
 * header of its own beside rmpc.h and rmpc_assign_opt.h: their entries are what they were.  Written in the forms
 * robot_mpcs_amd/_abi.py reads.
 *
 * rmpc_tours_device solves G independent problems: B robots, T tasks, at most K tasks per robot.  Per problem
 * d_start_cost [B][T] (fp64, robot to task) and d_task_cost [T][T] (fp64, task i to task j; it may be asymmetric, the
 * diagonal is never read).  It knows nothing of grids.  A heuristic on integers -- cheapest insertion, then the best
 * relocation or exchange per round -- with every choice a minimum under a strict total order, so that the result is
 * pinned bit for bit.
 *
 * Quantise.  Exactly as rmpc_assign_opt.h: r = rint(cost * scale), one fp64 product rounded half to even; an edge is
 * takeable when cost >= 0, cost < +inf and r <= RMPC_ASSIGN_OPT_MAX_Q, and its integer cost is q = (int) r.  An edge
 * that is not takeable is never used.  Below e(x, y) is the q of the edge from x (a robot's start or a task) to the
 * task y.
 *
 * State.  tour [b] is a sequence of at most K distinct tasks, empty at first; c [b] is the sum of q along
 * start_b -> tour [b][0] -> tour [b][1] -> ...  Tours are open: there is no return leg.  A position k of a tour of
 * length n, 0 <= k <= n, is the gap in front of its k-th task (behind the last one when k == n): its predecessor is the
 * start when k == 0, else tour [b][k - 1]; it has a successor when k < n.  Inserting t at a gap costs
 *   ins = e(pred, t) + (e(t, succ) - e(pred, succ) when there is a successor),
 * and both new edges must be takeable.  ins may be negative: the costs need not obey the triangle inequality.
 *
 * Build.  Repeat until no candidate is left; tasks that are never inserted stay unassigned.  A candidate is (b, t, k): t
 * unassigned, len(tour [b]) < K, k a position of tour [b], every new edge takeable; delta = ins.  The least candidate wins,
 *   mode 0 (least sum):       by (delta, b, t, k),
 *   mode 1 (least makespan):  by (c [b] + delta, b, t, k),
 * and is inserted; build_steps += 1.
 *
 * Improve.  Repeat while rounds < max_rounds.  The candidate moves:
 *   relocate (t, b2, k2): t is taken out of its tour b1 -- when it has a successor the bridging edge e(pred, succ) must
 *     be takeable; taking it out changes c [b1] by -rem, rem = e(pred, t) + (e(t, succ) - e(pred, succ) with a successor)
 *     -- and inserted at position k2 of tour [b2], or of the shortened tour [b1] when b2 == b1.  len(tour [b2]) < K is
 *     required when b2 != b1.  The no-op (b2 == b1 and k2 the position t came from) is excluded.
 *   exchange (ta < tb): two assigned tasks change places, in one tour or between two.  Every new edge must be takeable.
 * A move touches one or two tours.  ds is the change of the sum of their costs, pm_old the greatest cost of the touched
 * tours before the move, pm_new the greatest after it.  A move is admissible
 *   mode 0: when ds < 0;
 *   mode 1: when pm_new < pm_old, or pm_new == pm_old and ds < 0.
 * The admissible move that is least is applied; with none, stop.  A relocate has kind = 0 and (i, j, l) = (t, b2, k2), an
 * exchange kind = 1 and (ta, tb, 0);
 *   mode 0 orders by (ds, kind, i, j, l),
 *   mode 1 orders by (pm_new - pm_old, ds, kind, i, j, l);
 * rounds += 1.
 *
 * Termination.  mode 0: the integer sum of the tour costs falls strictly with every round and is bounded below by 0.
 * mode 1: the vector of tour costs sorted in descending order falls lexicographically with every round -- of the touched
 * tours either the greatest cost falls, or it stays and the other one falls (one touched tour with pm_new == pm_old has
 * ds == 0 and is not admissible) -- and there are finitely many such vectors.  So the makespan max c [b] never rises in
 * mode 1; the sum may rise.  The build ends after at most min(T, B K) steps.
 *
 * Bounds.  q <= 2^20 and a tour has at most K <= 1024 edges: 0 <= c [b] <= 2^30, |ins|, |rem| <= 3 * 2^20,
 * |ds| <= 6 * 2^20 < 2^23, |pm_new - pm_old| <= 2^30; the sum of all tours is at most 2^40.  The orders above need not
 * fit one 64-bit key; the kernels reduce in two steps, first the least leading part (delta, c + delta, ds or
 * (pm_new - pm_old, ds), biased to be non-negative), then the least index part among its equals.  The result is what is
 * pinned, not the representation.
 *
 * rmpc_follow_tour_device is rmpc_follow_path_device (rmpc.h) extended by stops; its rule stands at the declaration. */
#ifndef RMPC_TOURS_H
#define RMPC_TOURS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMPC_TOURS_MAX_ROBOTS 1024
#define RMPC_TOURS_MAX_TASKS 1024

/* The bytes of workspace rmpc_tours_device needs for G problems of B robots and T tasks: the quantised start costs, the
 * quantised task costs and their transpose, and per (robot, task) the cheapest insertion into the tour as it stands and
 * its position, int32 each: 4 G (3 B T + 2 T T).  Host only: no HIP call.  -1 (and a message in rmpc_last_error) on sizes
 * the entry refuses. */
int64_t rmpc_tours_work_bytes(int G, int B, int T);

/* d_start_cost [G][B][T], d_task_cost [G][T][T] fp64 -> d_tours [G][B][K] int32 (the tasks of every robot in order,
 * padded with -1), d_len [G][B] int32, d_cost [G][B] int64 (c [b]) and, where not NULL, d_owner [G][T] int32 (the robot
 * of every task, or -1), d_count [G] int32 (assigned tasks), d_total [G] int64 (the sum of c), d_span [G] int64 (the
 * greatest c), d_build_steps [G] int32, d_rounds [G] int32, by the rule above.
 * 1 <= B <= RMPC_TOURS_MAX_ROBOTS, 1 <= T <= RMPC_TOURS_MAX_TASKS, 1 <= K <= T, 1 <= G, G T T <= INT_MAX and
 * G B T <= INT_MAX; mode 0 or 1; scale finite and > 0; max_rounds >= 0; d_work: work_bytes >=
 * rmpc_tours_work_bytes(G, B, T) bytes of device memory, aligned to 4, whose prior contents are irrelevant.  Takes a
 * stream, allocates nothing, never synchronises, runs on the device of d_start_cost, leaves its inputs as they are.
 * Refused before any HIP call: a NULL d_start_cost, d_task_cost, d_tours, d_len, d_cost or d_work, sizes outside the
 * limits, a bad scale or mode, a negative max_rounds, work_bytes below the query. */
int rmpc_tours_device(int G, int B, int T, int K, const double *d_start_cost, const double *d_task_cost, int mode,
                      double scale, int max_rounds, int32_t *d_tours, int32_t *d_len, int64_t *d_cost, int32_t *d_owner,
                      int32_t *d_count, int64_t *d_total, int64_t *d_span, int32_t *d_build_steps, int32_t *d_rounds,
                      void *d_work, int64_t work_bytes, void *stream);

/* rmpc_follow_path_device with stops, for B robots in one control step.  d_path [B][max_len], d_len [B], d_idx [B],
 * d_pos, stride, W, x0, y0, cell, threshold and d_goal [B][3] as there.  d_stop_at [B][K] int32: ascending indices into
 * the robot's path, -1 for an unused entry; d_leg [B] int32, in and out: the number of stops served; d_served [B][K]
 * int32: entry (b, leg) is written once, with `now`, when that stop is served.  Per robot b with d_len [b] > 0, with
 * i = d_idx [b] (clamped to the path), leg = d_leg [b] (at least 0) and dist the distance from d_pos [b * stride + 0 .. 1]
 * to the centre of d_path [b][i]:
 *   when leg < K and d_stop_at [b][leg] == i: only when dist <= stop_tol, d_served [b][leg] = now, leg += 1, and i
 *     advances by one when i < d_len [b] - 1 and the next stop (leg < K) is not at i as well; otherwise nothing moves;
 *   when i is not a stop: i advances by one when i < d_len [b] - 1 and dist <= threshold.
 * Then d_goal [b] = (centre of d_path [b][i], 0).  One advance per call.  A robot with d_len [b] <= 0 keeps everything
 * it has.  Refused before any HIP call: a NULL pointer, B, max_len, K < 1, B max_len or B K above INT_MAX, stride < 2,
 * W < 1, a stop_tol that is negative or NaN. */
int rmpc_follow_tour_device(int B, const int32_t *d_path, const int32_t *d_len, int max_len, int32_t *d_idx,
                            const double *d_pos, int stride, int W, double x0, double y0, double cell, double threshold,
                            double *d_goal, int K, const int32_t *d_stop_at, int32_t *d_leg, int32_t *d_served, int now,
                            double stop_tol, void *stream);

#ifdef __cplusplus
}
#endif

#endif
