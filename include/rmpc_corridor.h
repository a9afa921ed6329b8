/* rmpc_corridor.h -- safe corridors from the map: for every robot and every stage of the coming solve a rectangle of
 * cells known to be free, written as four half-planes into the lin_constrs slots the LinearConstraints rows read
 * (DESIGN.md 29), a header of its own beside rmpc.h: the entries of rmpc.h are what they were.  Written in the forms
 * robot_mpcs_amd/_abi.py reads.  What decides is exact in integers; the doubles are formed in the order written here,
 * without contraction, so a plain restatement gives the same bits.
 *
 * Occupancy.  A grid is d_grid [H][W] doubles, cell (row, col); the centre of a cell is (x0 + col cell, y0 + row cell), so
 * the cell covers x0 + (col -+ 0.5) cell.  A cell is occupied when its value is not below occ_threshold, the any-angle
 * rule !(v < thr): a NaN counts as occupied.  S is the summed-area table of the occupancy, [H + 1][W + 1] int32:
 * row 0 and column 0 are 0, S [r + 1][c + 1] is the number of occupied cells in rows 0 .. r, columns 0 .. c.  The
 * count of the box of rows ra .. rb and columns ca .. cb is
 *   S [rb + 1][cb + 1] - S [ra][cb + 1] - S [rb + 1][ca] + S [ra][ca].
 *
 * Seed cell.  (r, c) of a point p is formed as rmpc_grid_cells_device forms a cell: c = rint((p [0] - x0) / cell),
 * r = rint((p [1] - y0) / cell), round half to even.  A coordinate that is not finite, or a cell outside the map, gives
 * status -1; a seed cell whose count is not 0 gives status 0; otherwise the status is 1.
 *
 * Growth (status 1).  r0 = r1 = r, c0 = c1 = c.  Rounds are repeated; a round tries the four directions in the order
 * +col, +row, -col, -row, each against the rectangle as the directions before it in the same round left it.  A
 * direction advances by one line when the new line lies inside the map, is at most reach cells from the seed
 * (c1 + 1 - c <= reach, r1 + 1 - r <= reach, c - (c0 - 1) <= reach, r - (r0 - 1) <= reach) and its count (the new column
 * over rows r0 .. r1, or the new row over columns c0 .. c1) is 0.  Growth stops after the first round in which no
 * direction advanced.  A line that is refused is refused in every later round (the rectangle only grows), so a
 * direction advances in consecutive rounds from the first: there are at most reach + 1 rounds.
 *
 * Planes (status 1), every operation in the order written:
 *   xlo = x0 + ((double)c0 - 0.5) * cell,  xhi = x0 + ((double)c1 + 0.5) * cell,
 *   ylo = y0 + ((double)r0 - 0.5) * cell,  yhi = y0 + ((double)r1 + 0.5) * cell;
 *   slot0 + 0: (1, 0, 0, -xlo)   slot0 + 1: (-1, 0, 0, xhi)   slot0 + 2: (0, 1, 0, -ylo)   slot0 + 3: (0, -1, 0, yhi),
 * the zeros +0.0.  A plane (a, d) holds a . p + d >= 0 inside.  The LinearConstraints row is |a . p + d| / |a| - r_body
 * >= 0: it takes the absolute value, so it keeps the collision point r_body from each face on the side the point is on
 * and does not know which side is inside.  The point is inside when the planes are written -- its own cell is part of
 * the rectangle --, and a plan that starts inside and keeps every row cannot cross a face; a seed closer than r_body to a
 * face of its rectangle (a point in the outer part of a cell whose neighbour is occupied) violates the row at once.
 *
 * Status <= 0.  The four slots get the dummy plane of the free-space decomposition around the point s = d_points [b][k]:
 * with q = s + (20, 20, 0) and n = s - q the plane (n, -((n0 q0 + n1 q1) + n2 q2)).  d_rect gets (-1, -1, -1, -1).  A
 * point that is not finite yields planes that are not finite, as the free-space decomposition does; keeping a NaN
 * input to its own instance stays the solver's business. */
#ifndef RMPC_CORRIDOR_H
#define RMPC_CORRIDOR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMPC_CORRIDOR_MAX_REACH 256         /* rmpc_grid_corridor_device: the most cells a side lies from its seed */
/* the bytes of d_sums: the summed-area table, [H + 1][W + 1] int32 */
#define RMPC_CORRIDOR_SUMS_BYTES(H, W) (4LL * ((long long)(H) + 1) * ((long long)(W) + 1))

/* d_grid [H][W] -> d_sums, RMPC_CORRIDOR_SUMS_BYTES(H, W) bytes whose prior contents are irrelevant: the table S above,
 * once per map.  H, W >= 1, H W <= RMPC_GRID_LARGE_MAX_CELLS (rmpc_grid_large.h).  Takes a stream, allocates nothing,
 * never synchronises, runs on the device of d_grid.  Refused before any HIP call: a NULL pointer, H or W < 1, a map
 * above the limit, an occ_threshold that is not finite. */
int rmpc_grid_occ_sums_device(int H, int W, const double *d_grid, double occ_threshold, int32_t *d_sums, void *stream);

/* d_points [B][N][3] (as rmpc_fleet_points_device writes them) -> slots slot0 .. slot0 + 3 of d_planes [B][N][nobst][4],
 * every other slot untouched; d_rect [B][N][4] int32 (r0, r1, c0, c1), inclusive, and d_status [B][N] int32 may be
 * NULL.  d_sums is what rmpc_grid_occ_sums_device wrote for the same H, W.  1 <= reach <= RMPC_CORRIDOR_MAX_REACH;
 * B, N >= 1; slot0 >= 0 and slot0 + 4 <= nobst; B N nobst 4 <= INT_MAX; cell finite and > 0, x0 and y0 finite; the map
 * as above.  Takes a stream, allocates nothing, never synchronises, runs on the device of d_sums.  Refused before any
 * HIP call: a NULL d_sums, d_points or d_planes and any violation of these limits. */
int rmpc_grid_corridor_device(int H, int W, const int32_t *d_sums, double x0, double y0, double cell, int B, int N,
                              const double *d_points, int reach, int nobst, int slot0, double *d_planes, int32_t *d_rect,
                              int32_t *d_status, void *stream);

#ifdef __cplusplus
}
#endif

#endif
