// rmpc_grid.hpp -- the global planner on the device (robotmpcs/global_planner/: occupancy map -> enlarged obstacles
// -> 8-connected shortest path -> waypoint follower), included by rmpc_world.hip.  Grids are [H][W] doubles, row-major,
// cell c = row * W + col; the plain frame puts the centre of (row, col) at (x0 + col * cell, y0 + row * cell).
//
// The field kernel builds one cost-to-go field per goal, D(goal) = 0, D(u) = min_v (delta(u, v) + E(v)) with
// E(v) = f data[v] + D(v) (the price of entering v, then the rest of the way), +inf on occupied and unreachable cells.
// Every update is a monotone min from +inf with the same floating-point expression, so any order of in-place updates
// reaches the same fixed point, the one a Dijkstra of this recursion computes ("Global planner").
// Contraction is off in every function here: fields, paths and the follower are bitwise those of a plain double
// restatement on the host.
//
// The seeded field (k_grid_fields_seeded) takes its sources from seeds [H][W] instead of one goal cell:
// D(u) = min(seed(u), min_v (delta(u, v) + E(v))), a seed of +inf is no source, a finite one a start potential.  It is
// the same recursion with a virtual source joined to every seeded cell by an edge of the seed's length, so the same
// argument gives the same fixed point; k_grid_descend walks such a field down to a source.

#include <climits>

namespace rmpc {

constexpr int kGridMaxCells = RMPC_GRID_MAX_CELLS;
constexpr int kGridThreads = 1024;                       // one workgroup per goal
constexpr int kGridPer = kGridMaxCells / kGridThreads + 1;   // most cells per thread (odd: see k_grid_fields)
constexpr double kSqrt2 = 1.4142135623730951;            // == math.sqrt(2)

// the reference's move order (a_star.py, _get_movements_8n; the first four are _get_movements_4n): (dcol, drow)
__device__ __forceinline__ int grid_dc(int m) { return m == 0 || m == 4 || m == 7 ? 1 : (m == 2 || m == 5 || m == 6 ? -1 : 0); }
__device__ __forceinline__ int grid_dr(int m) { return m == 1 || m == 4 || m == 5 ? 1 : (m == 3 || m == 6 || m == 7 ? -1 : 0); }
__device__ __forceinline__ double grid_delta(int m) { return m < 4 ? 1.0 : kSqrt2; }

// get_enlarged_obstacles: box mean over (2k+1)^2 on interior cells (convolution_size_robot), raw value within k of the
// border, then 1 above the threshold, 0 otherwise (create_binary_map)
__global__ __launch_bounds__(256) void k_grid_inflate(const double *__restrict__ in, double *__restrict__ out, int H, int W,
                                                      int k, double threshold) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= H * W) return;
  const int r = c / W, col = c - r * W;
  double v = in[c];
  if (r >= k && r < H - k && col >= k && col < W - k) {
    double s = 0.0;
    for (int i = r - k; i <= r + k; i++)
      for (int j = col - k; j <= col + k; j++) s += in[i * W + j];
    v = s / (double)((2 * k + 1) * (2 * k + 1));
  }
  out[c] = v > threshold ? 1.0 : 0.0;
}

// One workgroup per goal.  Thread t owns the cells t * per .. t * per + per - 1 (per = ceil(H W / 1024) rounded up to
// an odd number, <= 17): their D and neighbour masks stay in registers, E of every cell lives in LDS.  Sweeps alternate their direction within a
// thread's run and update in place; the loop ends after a sweep in which no thread lowered a value: all of E was
// constant during that sweep, so every thread checked every edge against final values -- the fixed point.
//
// kSeeded: the sources are the cells with a finite seeds [g][c] (a start potential >= 0) instead of goal_cells [g].  Every
// free cell takes part, a seeded one too: a neighbour may undercut its seed.  Only the set-up differs; the sweeps are
// the same code, so the goal variant's fields are what they were.
template <bool kSeeded>
__device__ __forceinline__ void grid_fields(const double *__restrict__ grid, int H, int W, const int *__restrict__ goal_cells,
                                            const double *__restrict__ seeds, int nmoves, double occ_threshold,
                                            double cost_factor, double *__restrict__ fields, int *__restrict__ status,
                                            int *__restrict__ sweeps) {
#pragma clang fp contract(off)
  __shared__ double E[kGridMaxCells];
  const int HW = H * W, g = blockIdx.x, t = threadIdx.x;
  // runs of an odd length: the 32 lanes of one LDS access are `per` doubles = 2 per banks apart, which for odd per puts
  // every lane on its own bank pair (per = 16 would put them on 2 pairs: a 16-way conflict on every read)
  const int per = ((HW + kGridThreads - 1) / kGridThreads) | 1;
  const int goal = kSeeded ? -1 : goal_cells[g];
  const bool goal_in = kSeeded || (goal >= 0 && goal < HW);
  const bool goal_ok = kSeeded || (goal_in && grid[goal] < occ_threshold);
  double *const F = fields + (size_t)g * HW;
  const double inf = __builtin_inf();
  if (!goal_ok) {
    for (int c = t; c < HW; c += kGridThreads) F[c] = inf;
    if (t == 0) { status[g] = goal_in ? RMPC_GRID_GOAL_OCCUPIED : RMPC_GRID_OUTSIDE; if (sweeps) sweeps[g] = 0; }
    return;
  }
  const double *const S = kSeeded ? seeds + (size_t)g * HW : nullptr;
  double D[kGridPer];
  bool bad = false;           // a free cell with a negative value (a negative price would make the sweeps diverge)
  bool bad_seed = false;      // a free cell with a negative or NaN seed
  // per cell 10 bits, three cells to a register: bit m = neighbour m inside the map, bit 8 = the cell takes part (owned,
  // free, not the goal)
  unsigned fw[(kGridPer + 2) / 3];
#pragma unroll
  for (int w = 0; w < (kGridPer + 2) / 3; w++) fw[w] = 0;
#define RMPC_GRID_FLAGS(i) ((fw[(i) / 3] >> (10 * ((i) % 3))) & 1023u)
#pragma unroll
  for (int i = 0; i < kGridPer; i++) {
    const int c = t * per + i;
    D[i] = inf;
    if (i < per && c < HW) {
      const double d = grid[c];
      const int r = c / W, col = c - r * W;
      unsigned f = 0;
      for (int m = 0; m < nmoves; m++) {
        const int rr = r + grid_dr(m), cc = col + grid_dc(m);
        if (rr >= 0 && rr < H && cc >= 0 && cc < W) f |= 1u << m;
      }
      if constexpr (kSeeded) {
        const bool is_free = d < occ_threshold;
        const double s = is_free ? S[c] : inf;        // a seed on an occupied cell is ignored
        bad_seed = bad_seed || !(s >= 0.0);
        D[i] = s;
        if (is_free) f |= 256u;
        E[c] = s < inf ? cost_factor * d + s : inf;
      } else {
        if (c == goal) D[i] = 0.0;
        else if (d < occ_threshold) f |= 256u;
        E[c] = c == goal ? cost_factor * d + 0.0 : inf;
      }
      bad = bad || (d < occ_threshold && !(d >= 0.0));
      fw[i / 3] |= f << (10 * (i % 3));
    }
  }
  if (__syncthreads_or(bad)) {
    for (int c = t; c < HW; c += kGridThreads) F[c] = inf;
    if (t == 0) { status[g] = RMPC_GRID_BAD_MAP; if (sweeps) sweeps[g] = 0; }
    return;
  }
  if constexpr (kSeeded) {
    if (__syncthreads_or(bad_seed)) {
      for (int c = t; c < HW; c += kGridThreads) F[c] = inf;
      if (t == 0) { status[g] = RMPC_GRID_BAD_SEED; if (sweeps) sweeps[g] = 0; }
      return;
    }
  }
  // one cell of a sweep; the price f data[u] is read again only when D(u) drops (L1 / L2 hits), which keeps the
  // thread's D and flags in registers without scratch
  double *const Et = E + t * per;
  const double *const gt = grid + t * per;
  auto relax = [&](int i, bool &lowered) {
    const unsigned flags = RMPC_GRID_FLAGS(i);
    if (flags & 256u) {
      double best = D[i];
#pragma unroll
      for (int m = 0; m < 8; m++)
        if (flags & (1u << m)) {
          const double cand = grid_delta(m) + Et[i + grid_dr(m) * W + grid_dc(m)];
          best = cand < best ? cand : best;
        }
      if (best < D[i]) {
        D[i] = best;
        Et[i] = cost_factor * gt[i] + best;
        lowered = true;
      }
    }
  };
  // With prices >= 0 (cost_factor >= 0 checked on the host, free cells >= 0 above) every sweep does at least one Jacobi
  // step, so a field is final after at most H W sweeps (the depth of its shortest-path tree) plus the quiet one.  The
  // bound only guards against inputs those checks do not foresee: the loop never runs unbounded.
  int sweep = 0;
  bool converged = false;
  for (; sweep <= HW; sweep++) {
    bool lowered = false;
    if (sweep & 1) {
#pragma unroll
      for (int i = kGridPer - 1; i >= 0; i--) relax(i, lowered);
    } else {
#pragma unroll
      for (int i = 0; i < kGridPer; i++) relax(i, lowered);
    }
    if (!__syncthreads_or(lowered)) { converged = true; break; }
  }
#pragma unroll
  for (int i = 0; i < kGridPer; i++) {
    const int c = t * per + i;
    if (i < per && c < HW) F[c] = converged ? D[i] : inf;
  }
#undef RMPC_GRID_FLAGS
  if (t == 0) {
    status[g] = converged ? RMPC_GRID_OK : RMPC_GRID_NO_FIXED_POINT;
    if (sweeps) sweeps[g] = converged ? sweep + 1 : sweep;
  }
}

__global__ __launch_bounds__(kGridThreads) void k_grid_fields(const double *__restrict__ grid, int H, int W,
                                                              const int *__restrict__ goal_cells, int nmoves,
                                                              double occ_threshold, double cost_factor,
                                                              double *__restrict__ fields, int *__restrict__ status,
                                                              int *__restrict__ sweeps) {
  grid_fields<false>(grid, H, W, goal_cells, nullptr, nmoves, occ_threshold, cost_factor, fields, status, sweeps);
}

__global__ __launch_bounds__(kGridThreads) void k_grid_fields_seeded(const double *__restrict__ grid, int H, int W,
                                                                     const double *__restrict__ seeds, int nmoves,
                                                                     double occ_threshold, double cost_factor,
                                                                     double *__restrict__ fields, int *__restrict__ status,
                                                                     int *__restrict__ sweeps) {
  grid_fields<true>(grid, H, W, nullptr, seeds, nmoves, occ_threshold, cost_factor, fields, status, sweeps);
}

// descent of field goal_index[b] from start_cell[b]: the neighbour with the least delta + f data[v] + D(v), the first in
// move order on ties, until the goal
__global__ __launch_bounds__(256) void k_grid_paths(const double *__restrict__ grid, int H, int W, const double *__restrict__ fields,
                                                    const int *__restrict__ goal_cells, int G, const int *__restrict__ start_cell,
                                                    const int *__restrict__ goal_index, int B, int nmoves, double occ_threshold,
                                                    double cost_factor, int max_len, int *__restrict__ path, int *__restrict__ len) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int HW = H * W, s = start_cell[b], gi = goal_index[b];
  const int goal = gi >= 0 && gi < G ? goal_cells[gi] : -1;
  int *const out = path + (size_t)b * max_len;
  if (s < 0 || s >= HW || goal < 0 || goal >= HW) { len[b] = RMPC_GRID_OUTSIDE; return; }
  if (!(grid[s] < occ_threshold)) { len[b] = RMPC_GRID_START_OCCUPIED; return; }
  if (!(grid[goal] < occ_threshold)) { len[b] = RMPC_GRID_GOAL_OCCUPIED; return; }
  const double *const F = fields + (size_t)gi * HW;
  if (!(F[s] < __builtin_inf())) { len[b] = 0; return; }
  int u = s, n = 0;
  for (;;) {
    if (n >= max_len) { len[b] = RMPC_GRID_TOO_LONG; return; }
    out[n++] = u;
    if (u == goal) break;
    const int r = u / W, col = u - r * W;
    double best = __builtin_inf();
    int next = -1;
    for (int m = 0; m < nmoves; m++) {
      const int rr = r + grid_dr(m), cc = col + grid_dc(m);
      if (rr < 0 || rr >= H || cc < 0 || cc >= W) continue;
      const int v = rr * W + cc;
      const double cand = grid_delta(m) + (cost_factor * grid[v] + F[v]);
      if (cand < best) { best = cand; next = v; }
    }
    if (next < 0) { len[b] = 0; return; }   // (not reached on a field of this grid: D(u) finite has a finite neighbour)
    u = next;
  }
  len[b] = n;
}

// descent of the seeded field field_index[b] from start_cell[b] by the step rule of k_grid_paths, until the first cell u
// with D(u) finite and D(u) == seed(u): a source that nothing undercuts (an undercut one is passed through).  The start
// cell is not tested for occupancy -- a robot stands where it stands: from a start with D = +inf the first step goes to
// the best neighbour, and the length is 0 when none is finite.  Every later cell has a finite D, which falls strictly
// along the walk; max_len bounds the loop whatever the field holds.
__global__ __launch_bounds__(256) void k_grid_descend(const double *__restrict__ grid, int H, int W, const double *__restrict__ fields,
                                                      const double *__restrict__ seeds, int G, const int *__restrict__ start_cell,
                                                      const int *__restrict__ field_index, int B, int nmoves, double occ_threshold,
                                                      double cost_factor, int max_len, int *__restrict__ path, int *__restrict__ len) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int HW = H * W, s = start_cell[b], fi = field_index[b];
  int *const out = path + (size_t)b * max_len;
  if (s < 0 || s >= HW || fi < 0 || fi >= G) { len[b] = RMPC_GRID_OUTSIDE; return; }
  const double *const F = fields + (size_t)fi * HW, *const S = seeds + (size_t)fi * HW;
  int u = s, n = 0;
  for (;;) {
    if (n >= max_len) { len[b] = RMPC_GRID_TOO_LONG; return; }
    const double Du = F[u];
    const bool source = Du < __builtin_inf() && Du == S[u];
    int next = -1;
    if (!source) {
      const int r = u / W, col = u - r * W;
      double best = __builtin_inf();
      for (int m = 0; m < nmoves; m++) {
        const int rr = r + grid_dr(m), cc = col + grid_dc(m);
        if (rr < 0 || rr >= H || cc < 0 || cc >= W) continue;
        const int v = rr * W + cc;
        if (!(grid[v] < occ_threshold)) continue;
        const double cand = grid_delta(m) + (cost_factor * grid[v] + F[v]);
        if (cand < best) { best = cand; next = v; }
      }
      if (next < 0) { len[b] = 0; return; }   // only at the start: walled in, or no source reaches it
    }
    out[n++] = u;
    if (source) break;
    u = next;
  }
  len[b] = n;
}

// world position (pointer + stride) -> cell of the plain frame, -1 outside: rint = round half to even, as Python's round
// in gridmap.get_index_from_coordinates
__global__ __launch_bounds__(256) void k_grid_cells(const double *__restrict__ pos, int stride, int B, int H, int W, double x0,
                                                    double y0, double cell, int *__restrict__ cells) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double fc = rint((pos[(size_t)b * stride] - x0) / cell), fr = rint((pos[(size_t)b * stride + 1] - y0) / cell);
  cells[b] = fc >= 0.0 && fc < (double)W && fr >= 0.0 && fr < (double)H ? (int)fr * W + (int)fc : -1;
}

// get_local_goal for B robots: one step along the path when the current waypoint is within threshold and it is not
// the last one, then the waypoint's centre becomes the scene's goal
__global__ __launch_bounds__(256) void k_follow_path(const int *__restrict__ path, const int *__restrict__ len, int max_len,
                                                     int *__restrict__ idx, const double *__restrict__ pos, int stride, int B,
                                                     int W, double x0, double y0, double cell, double threshold,
                                                     double *__restrict__ goal) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int L = len[b];
  if (L <= 0) return;
  const int *const p = path + (size_t)b * max_len;
  int i = idx[b];
  i = i < 0 ? 0 : (i >= L ? L - 1 : i);
  int c = p[i];
  double cx = x0 + (double)(c % W) * cell, cy = y0 + (double)(c / W) * cell;
  const double dx = cx - pos[(size_t)b * stride], dy = cy - pos[(size_t)b * stride + 1];
  if (i < L - 1 && sqrt(dx * dx + dy * dy) <= threshold) {
    i++;
    c = p[i];
    cx = x0 + (double)(c % W) * cell;
    cy = y0 + (double)(c / W) * cell;
  }
  idx[b] = i;
  goal[(size_t)b * 3] = cx;
  goal[(size_t)b * 3 + 1] = cy;
  goal[(size_t)b * 3 + 2] = 0.0;
}

}  // namespace rmpc
