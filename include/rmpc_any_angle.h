/* rmpc_any_angle.h -- line of sight on the grid, routes shortened by it and a follower whose look-ahead goal is the
 * farthest route cell the robot can see, a header of its own beside rmpc.h: the entries of rmpc.h are
 * what they were.  Written in the forms robot_mpcs_amd/_abi.py reads.  Everything here is exact in integers.
 *
 * Visible.  A grid is d_grid [H][W] doubles, cell = row * W + col; a cell is occupied when its value is not below
 * occ_threshold, the planner's test (data >= occ_threshold; a NaN counts as occupied).  For two cells a and b take the
 * closed segment between their centres, in cell units.  A cell is touched when its closed unit square meets that
 * segment: a segment through a lattice corner touches all four cells round it, so both side cells count and no corner
 * is cut.  visible(a, b) holds when no touched cell other than a is occupied.  a is exempt -- a robot stands where it
 * stands --, b is not; visible(a, a) holds.  The touched cells lie in the bounding box of a and b: nothing outside
 * the map is read.  The touched cells are enumerated by an integer walk from a to b:
 *   dx = |col b - col a|, dy = |row b - row a|, e = dx - dy, n = dx + dy, then dx and dy are doubled;
 *   while n > 0:  e > 0: one step in x, e -= dy, n -= 1;
 *                 e < 0: one step in y, e += dx, n -= 1;
 *                 e == 0 (the segment passes a lattice corner): the two side cells (x stepped alone, y stepped
 *                         alone) are tested, then one step in both, e += dx - dy, n -= 2;
 *                 the cell stepped into is tested.
 * The walk takes at most dx + dy steps and ends at the first occupied cell it tests.
 *
 * Shorten: string pulling by line of sight, a greedy heuristic and not an optimal any-angle path.  Per path
 * p [0 .. L), L = d_len [b]:  out [0] = p [0], i = 0;  while i < L - 1:  hi = min(L - 1, i + reach) (reach == 0 means
 * L - 1) and, with d_keep, no larger than the first k > i with keep [k] != 0;  j = the largest index in (i, hi] with
 * j == i + 1 or visible(p [i], p [j]);  p [j] is appended, i = j.  The path's own next cell is always accepted: a dense
 * path may take a diagonal between two occupied cells, which is not visible.  Repeated cells collapse (a cell sees
 * itself), so this is not for timed paths, whose order of passage depends on every waypoint.
 *
 * Follow visible: one control step of a follower per robot with L = d_len [b] > 0.  i = d_idx [b] clamped to
 * [0, L - 1]; s = the robot's cell as rmpc_grid_cells_device forms it (rint, -1 outside).  With s >= 0, j is the
 * largest k in [i, min(L - 1, i + reach)] with  sqrt(dx dx + dy dy) <= look_ahead  from the robot's position to the
 * centre of p [k] (the expressions and the order of rmpc_follow_path_device, no contraction),  p [k] inside the map
 * and  visible(s, p [k]);  without such a k, and with s < 0, j = i.  Then d_idx [b] = j and
 * d_goal [b] = (centre of p [j], 0) as rmpc_follow_path_device writes it; d_blocked [b] = 1 when no k qualified, else
 * 0: the hook for a re-plan.  d_idx never decreases.  A robot with L <= 0 keeps everything it has.  look_ahead >= 2 cell:
 * a robot that converges on p [i] is then within reach of p [i + 1], an 8-connected neighbour, and cannot stall on the
 * distance test. */
#ifndef RMPC_ANY_ANGLE_H
#define RMPC_ANY_ANGLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMPC_VISIBLE_MAX_REACH 64           /* rmpc_follow_visible_device: one lane of a wavefront per candidate */
/* the bytes of d_work of rmpc_grid_shorten_device: the map's occupancy as bit rows, one 32-bit word per 32 cells of a row */
#define RMPC_SHORTEN_WORK_BYTES(H, W) (4LL * (long long)(H) * (((long long)(W) + 31) / 32))

/* d_from, d_to [P] int32 cells -> d_visible [P] int32: 1 visible, 0 not, -1 when either cell lies outside [0, H W).
 * H, W >= 1, H W <= RMPC_GRID_LARGE_MAX_CELLS (rmpc_grid_large.h), P >= 1.  Takes a stream, allocates nothing, never
 * synchronises, runs on the device of d_grid.  Refused before any HIP call: a NULL pointer, H, W or P < 1, a map
 * above the limit. */
int rmpc_grid_visible_device(int H, int W, const double *d_grid, double occ_threshold, int P, const int32_t *d_from,
                             const int32_t *d_to, int32_t *d_visible, void *stream);

/* d_path [B][max_len] int32, d_len [B] int32 (as rmpc_grid_paths_device writes them) -> d_out [B][max_len],
 * d_out_len [B] in the same layout, and, where not NULL, d_src [B][max_len]: the index in the input path of every
 * kept cell.  d_keep [B][max_len] int32 (may be NULL): a cell with a flag other than 0 is never skipped.
 * d_len [b] <= 0 passes through as d_out_len [b]; d_len [b] > max_len gives RMPC_GRID_TOO_LONG, a cell of the path
 * outside [0, H W) RMPC_GRID_OUTSIDE; none of these rows writes a cell.  Cells past d_out_len [b] are not written.
 * d_out may not be d_path.  d_work: RMPC_SHORTEN_WORK_BYTES(H, W) bytes of device memory, aligned to 4, whose prior
 * contents are irrelevant.  0 <= reach, B, max_len >= 1, B max_len <= INT_MAX, the map as above.  Takes a stream,
 * allocates nothing, never synchronises, runs on the device of d_grid.  Refused before any HIP call: a NULL d_grid,
 * d_path, d_len, d_out, d_out_len or d_work, d_out == d_path, sizes outside the limits, a negative reach. */
int rmpc_grid_shorten_device(int H, int W, const double *d_grid, double occ_threshold, int B, const int32_t *d_path,
                             const int32_t *d_len, int max_len, int reach, const int32_t *d_keep, int32_t *d_out,
                             int32_t *d_out_len, int32_t *d_src, void *d_work, void *stream);

/* One control step of the follower above for B robots.  d_path, d_len, max_len, d_idx, d_pos, stride, x0, y0, cell
 * and d_goal [B][3] as rmpc_follow_path_device; d_blocked [B] int32 may be NULL.  1 <= reach <= RMPC_VISIBLE_MAX_REACH;
 * cell and look_ahead finite and > 0, look_ahead >= 2 cell.  Runs on the device of d_path.  Refused before any HIP
 * call: a NULL pointer (d_blocked apart), B, max_len, H or W < 1, B max_len or B stride above INT_MAX, a map above the
 * limit, stride < 2, reach outside its range, a bad cell or look_ahead. */
int rmpc_follow_visible_device(int B, const int32_t *d_path, const int32_t *d_len, int max_len, int32_t *d_idx,
                               const double *d_pos, int stride, int H, int W, const double *d_grid, double occ_threshold,
                               double x0, double y0, double cell, int reach, double look_ahead, double *d_goal,
                               int32_t *d_blocked, void *stream);

#ifdef __cplusplus
}
#endif

#endif
