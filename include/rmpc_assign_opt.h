/* rmpc_assign_opt.h -- minimum-cost assignment of robots to targets on the device, a header of its own
 * beside rmpc.h: the entries of rmpc.h are what they were.  Written in the forms robot_mpcs_amd/_abi.py reads.
 *
 * rmpc_assign_optimal_device solves G independent problems d_cost [G][B][T] (fp64, any matrix: it knows nothing of
 * grids) by shortest augmenting paths on integers, so that the result is pinned bit for bit.
 *
 * Quantise.  r = rint(cost * scale): one fp64 product, rounded half to even.  A pair is takeable when cost >= 0,
 * cost < +inf and r <= RMPC_ASSIGN_OPT_MAX_Q; its integer cost is q = (int) r.  NaN, negative, +inf and too-large
 * entries are never taken.
 *
 * Orient.  The rows are the robots when B <= T, otherwise the targets: m = min(B, T) rows, n = max(B, T) columns.
 * Qmax is the greatest takeable q of the problem (0 when there is none), P = m Qmax + 1, and C [i][j] = q of the pair
 * when it is takeable, else P.  P <= 1024 * 2^20 + 1 = 2^30 + 1 fits an int32.
 *
 * Solve.  Rows in ascending order, the lowest column on every tie (rows and columns count from 1 here; column 0 is the
 * root of the search):
 *   u [0..m] = 0, v [0..n] = 0, p [0..n] = 0 (the row of a column, 0 = none)
 *   for i = 1 .. m:
 *     p [0] = i; j0 = 0; minv [1..n] = BIG; used [0..n] = false
 *     repeat                                                       -- one "step"
 *       used [j0] = true; i0 = p [j0]
 *       for every column j >= 1 not used: cur = C [i0][j] - u [i0] - v [j]; if cur < minv [j]: minv [j] = cur, way [j] = j0
 *       j1 = the unused column with the least (minv [j], j); delta = minv [j1]
 *       for used j: u [p [j]] += delta, v [j] -= delta;  for unused j: minv [j] -= delta
 *       j0 = j1
 *     until p [j0] == 0
 *     while j0 != 0: j1 = way [j0]; p [j0] = p [j1]; j0 = j1
 *
 * Report.  d_assign [G][B]: the target of the robot when its matched pair is takeable, else -1.  d_total [G]: the sum
 * of q over the assigned pairs; d_count [G]: their number; d_steps [G]: the steps of the loop above.
 *
 * What the result is.  Among all matchings that use takeable pairs only it has the greatest number of pairs and, among
 * those, the least sum of q: the loop minimises the sum of C over the matchings of all m rows, a matching with k
 * untakeable pairs costs k P + (a sum of at most m - 1 values q <= Qmax), and P > m Qmax, so one pair more always
 * pays.  Which of several optimal matchings comes out is fixed by the order above.
 *
 * Bounds (any 1 <= m <= n, 0 <= C <= Cmax; here m <= 1024, Cmax = 2^30 + 1).  The loop keeps u [i] + v [j] <= C [i][j]
 * for every row and column, with equality on matched pairs, and delta >= 0: u never falls, v never rises, so u >= 0
 * and v <= 0.  A column that no row holds has never been used, so its v is 0, and while the loop runs there is always
 * one (fewer than m <= n rows are matched): u [i] <= C [i][that column] <= Cmax.  A matched column has
 * v [j] = C [p [j]][j] - u [p [j]] >= -Cmax.  Hence 0 <= u <= Cmax, -Cmax <= v <= 0 and
 * 0 <= cur, minv, delta <= 2 Cmax = 2^31 + 2: every quantity fits 33 bits, whatever m is.  The worst case: rows 1 and
 * 2 are (0, Cmax, Cmax), row 3 is (Cmax, Cmax, Cmax); row 2 drives u [1] to Cmax and v [1] to -Cmax, and row 3 then
 * meets cur = 2 Cmax in column 1.  The argmin runs on the key minv * 2^13 + j (j <= 4096 < 2^13), below 2^45; BIG is
 * 2^62 and is overwritten in the first step of every row.  The kernels compute in int64. */
#ifndef RMPC_ASSIGN_OPT_H
#define RMPC_ASSIGN_OPT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMPC_ASSIGN_OPT_MAX_Q 1048576   /* 1 << 20: the greatest integer cost of a takeable pair */

/* The bytes of workspace rmpc_assign_optimal_device needs for G problems of B x T.  Host only: no HIP call.  -1 (and a
 * message in rmpc_last_error) on sizes the entry refuses. */
int64_t rmpc_assign_optimal_work_bytes(int G, int B, int T);

/* d_cost [G][B][T] fp64 -> d_assign [G][B] int32 and, where not NULL, d_total [G] int64, d_count [G] int32,
 * d_steps [G] int32, by the rule above.  1 <= B <= RMPC_ASSIGN_MAX_ROBOTS, 1 <= T <= RMPC_ASSIGN_MAX_TARGETS (rmpc.h),
 * 1 <= G and G B T <= INT_MAX; scale finite and > 0; d_work: work_bytes >= rmpc_assign_optimal_work_bytes(G, B, T)
 * bytes of device memory, aligned to 8, whose prior contents are irrelevant.  Takes a stream, allocates nothing, never
 * synchronises, runs on the device of d_cost, leaves d_cost as it is.  Refused before any HIP call: NULL d_cost,
 * d_assign or d_work, sizes outside the limits, a bad scale, work_bytes below the query. */
int rmpc_assign_optimal_device(int G, int B, int T, const double *d_cost, double scale, int32_t *d_assign,
                               int64_t *d_total, int32_t *d_count, int32_t *d_steps, void *d_work,
                               int64_t work_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
