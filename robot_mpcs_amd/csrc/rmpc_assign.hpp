// rmpc_assign.hpp -- coordinated exploration on the device, included by rmpc_world.hip behind
// rmpc_grid.hpp: the frontier cut into one target per tile (k_grid_targets), the route cost of every robot-target pair
// read off the targets' cost-to-go fields (k_grid_route_costs), and the greedy assignment of robots to targets
// (k_assign_greedy), which knows nothing of grids.  Every choice is a minimum under a strict total order of integers or
// of non-negative doubles compared by their bits, so no result depends on the order in which lanes meet.  Contraction
// is off in every function here, as in rmpc_grid.hpp.

namespace rmpc {

constexpr int kAssignMaxRobots = RMPC_ASSIGN_MAX_ROBOTS;
constexpr int kAssignMaxTargets = RMPC_ASSIGN_MAX_TARGETS;
constexpr int kAssignThreads = 1024;                      // one workgroup does the whole assignment
constexpr unsigned long long kAssignNoKey = ~0ull;        // above the bits of every takeable cost
static_assert(kAssignMaxTargets <= kAssignThreads && kAssignMaxTargets == 1024 && kAssignMaxRobots <= (1 << 21),
              "k_assign_greedy: a thread per target, (pass << 10 | target) in an int");

// One workgroup per tile of tile x tile cells (edge tiles are smaller), ntc tiles per row of tiles.  The sources of the
// tile are its cells with seed < +inf: n of them, rows summing to Sr, columns to Sc (integer adds).  The target is the
// source nearest their centroid, the least (n r - Sr)^2 + (n c - Sc)^2 in int64 (below 2^57 on a map of at most
// RMPC_GRID_MAX_CELLS cells), the lower cell on ties: the least distance by a 64-bit minimum, then the least cell among
// the sources that have it.  target_cells [t] = that cell or -1; tseeds [t] (when given) is written completely.
__global__ __launch_bounds__(256) void k_grid_targets(int H, int W, const double *__restrict__ seed, int tile, int ntc,
                                                      int *__restrict__ target_cells, double *__restrict__ tseeds) {
#pragma clang fp contract(off)
  __shared__ int s_n, s_r, s_c, s_cell;
  __shared__ unsigned long long s_d;
  const int t = blockIdx.x, tid = threadIdx.x;
  const int r0 = (t / ntc) * tile, c0 = (t % ntc) * tile;            // < H, < W: t < ntr * ntc
  const int h = tile > H - r0 ? H - r0 : tile, w = tile > W - c0 ? W - c0 : tile;
  const double inf = __builtin_inf();
  if (tid == 0) { s_n = 0; s_r = 0; s_c = 0; s_cell = INT_MAX; s_d = kAssignNoKey; }
  __syncthreads();
  int n = 0, sr = 0, sc = 0;
  for (int i = tid; i < h * w; i += 256) {
    const int r = r0 + i / w, c = c0 + i % w;
    if (seed[r * W + c] < inf) { n++; sr += r; sc += c; }
  }
  if (n) { atomicAdd(&s_n, n); atomicAdd(&s_r, sr); atomicAdd(&s_c, sc); }
  __syncthreads();
  const long long N = s_n, Sr = s_r, Sc = s_c;
  unsigned long long best = kAssignNoKey;
  int cell = INT_MAX;
  if (n)                                                             // (only a thread that saw a source sees one again)
    for (int i = tid; i < h * w; i += 256) {
      const int r = r0 + i / w, c = c0 + i % w;
      if (seed[r * W + c] < inf) {
        const long long dr = N * r - Sr, dc = N * c - Sc;
        const unsigned long long d = (unsigned long long)(dr * dr + dc * dc);
        if (d < best) { best = d; cell = r * W + c; }               // cells ascend within a thread: the lower one stays
      }
    }
  if (n) atomicMin(&s_d, best);
  __syncthreads();
  if (n && best == s_d) atomicMin(&s_cell, cell);
  __syncthreads();
  const int target = N > 0 ? s_cell : -1;
  if (tid == 0) target_cells[t] = target;
  if (tseeds) {
    double *const S = tseeds + (size_t)t * H * W;
    for (int c = tid; c < H * W; c += 256) S[c] = c == target ? 0.0 : inf;
  }
}

// One lane per (robot b, target t): the cost of the route from start_cell [b] down field t.  A start with D = +inf is
// priced by the start rule of k_grid_descend: the best free neighbour inside the map, in that kernel's expression.
__global__ __launch_bounds__(256) void k_grid_route_costs(const double *__restrict__ grid, int H, int W, int T,
                                                          const double *__restrict__ fields, int B,
                                                          const int *__restrict__ start_cell, int nmoves,
                                                          double occ_threshold, double cost_factor,
                                                          double *__restrict__ cost) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * T) return;
  const int b = i / T, t = i - b * T, u = start_cell[b];
  const double inf = __builtin_inf();
  double best = inf;
  if (u >= 0 && u < H * W) {
    const double *const F = fields + (size_t)t * H * W;
    best = F[u];
    if (!(best < inf)) {
      best = inf;
      const int r = u / W, col = u - r * W;
      for (int m = 0; m < nmoves; m++) {
        const int rr = r + grid_dr(m), cc = col + grid_dc(m);
        if (rr < 0 || rr >= H || cc < 0 || cc >= W) continue;
        const int v = rr * W + cc;
        if (!(grid[v] < occ_threshold)) continue;
        const double cand = grid_delta(m) + (cost_factor * grid[v] + F[v]);
        if (cand < best) best = cand;
      }
    }
  }
  cost[i] = best;
}

// the order of a takeable cost (>= 0 and < +inf; NaN fails both) as an integer: the bits of a non-negative double
// ascend with its value, and c + 0.0 takes -0.0 to +0.0, which compares equal to it
__device__ __forceinline__ unsigned long long assign_key(double c) {
#pragma clang fp contract(off)
  return c >= 0.0 && c < __builtin_inf() ? (unsigned long long)__double_as_longlong(c + 0.0) : kAssignNoKey;
}

// Greedy assignment of B robots to T targets in passes (include/rmpc.h), one workgroup.  Under the strict order
// (cost, b, t) a pair that is the least of its row and of its column among the remaining pairs is taken by the
// sequential rule before any other pair of its robot or target, so a round takes all such pairs at once.
//
// A round is driven by the columns, a thread per target:
//   A. colbest [t], the least (cost, b) over the free robots of an available target, is looked for again only when the
//      robot it names has been taken (robots only ever leave, so a cached best whose robot is free is still the best;
//      "none" stays none).  All such columns are scanned in one linear sweep of the matrix: thread i reads the elements
//      i, i + S T, i + 2 S T, ... with S = 1024 / T rows per step, all of one column i % T, so a wave reads consecutive
//      doubles; rows of taken robots and columns that need nothing are skipped.  The S partial minima of a column meet
//      in LDS: a 64-bit minimum of the cost's bits, then the least robot among those that have it.
//   B. only the rows that some colbest names can hold a dominant pair: those whose cached best is not of this pass or
//      has been taken are listed (once each);
//   C. a group of g = min(64, T rounded up to a power of two) lanes scans each listed row over the available targets;
//   D. target t takes robot b = colbest [t] when rowinfo [b] names t.
// rowinfo [b] = pass << 10 | target (-1 never scanned, -2 listed): a taken robot keeps the word it was taken with, which
// is what the kernel writes out at its end.  A pass ends with a round that takes nothing or leaves no target or no free
// robot; the next one makes every target available again and keeps the columns' cache.
__global__ __launch_bounds__(kAssignThreads) void k_assign_greedy(int B, int T, const double *__restrict__ cost,
                                                                   int *__restrict__ assign, int *__restrict__ pass_out) {
#pragma clang fp contract(off)
  __shared__ unsigned long long colkey[kAssignMaxTargets];
  __shared__ int colbest[kAssignMaxTargets], colnew[kAssignMaxTargets], rowlist[kAssignMaxTargets];
  __shared__ int rowinfo[kAssignMaxRobots];
  __shared__ unsigned char freeb[kAssignMaxRobots], avail[kAssignMaxTargets], need[kAssignMaxTargets];
  __shared__ int nlist;
  const int tid = threadIdx.x;
  const int S = kAssignThreads / T;                          // rows per step of the sweep, >= 1
  const bool sweeps = tid < S * T;
  const int st = tid % T, ss = tid / T;                      // the sweep's column and first row of this thread
  int g = 1;
  while (g < T && g < 64) g <<= 1;
  const int ngroups = kAssignThreads / g, group = tid / g, gl = tid % g;
  for (int b = tid; b < B; b += kAssignThreads) { freeb[b] = 1; rowinfo[b] = -1; }
  if (tid < T) { avail[tid] = 1; colbest[tid] = -1; }
  if (tid == 0) nlist = 0;
  int nfree = B, pass = 0;
  for (;;) {
    int navail = T, taken_in_pass = 0;
    for (;;) {
      // A
      bool mine = false;
      if (tid < T) {
        const int cb = colbest[tid];
        mine = avail[tid] && (cb == -1 || (cb >= 0 && !freeb[cb]));
        need[tid] = mine;
        if (mine) { colkey[tid] = kAssignNoKey; colnew[tid] = INT_MAX; }
      }
      if (__syncthreads_or(mine)) {
        unsigned long long best = kAssignNoKey;
        int bb = INT_MAX;
        if (sweeps && need[st]) {
          const double *const col = cost + st;
#pragma unroll 4
          for (int b = ss; b < B; b += S)
            if (freeb[b]) {
              const unsigned long long k = assign_key(col[(size_t)b * T]);
              if (k < best) { best = k; bb = b; }          // rows ascend within a thread: the lower one stays
            }
          if (best != kAssignNoKey) atomicMin(&colkey[st], best);
        }
        __syncthreads();
        if (best != kAssignNoKey && best == colkey[st]) atomicMin(&colnew[st], bb);
        __syncthreads();
        if (mine) colbest[tid] = colnew[tid] == INT_MAX ? -2 : colnew[tid];
      }
      // B
      const int mb = tid < T && avail[tid] ? colbest[tid] : -2;
      if (mb >= 0) {
        const int ri = rowinfo[mb];
        if (!(ri >= 0 && (ri >> 10) == pass && avail[ri & 1023]) && atomicExch(&rowinfo[mb], -2) != -2)
          rowlist[atomicAdd(&nlist, 1)] = mb;
      }
      __syncthreads();
      // C
      const int n = nlist;
      for (int i0 = 0; i0 < n; i0 += ngroups) {
        const int b = i0 + group < n ? rowlist[i0 + group] : -1;
        unsigned long long best = kAssignNoKey;
        int bt = INT_MAX;
        if (b >= 0) {
          const double *const row = cost + (size_t)b * T;
          for (int t = gl; t < T; t += g)
            if (avail[t]) {
              const unsigned long long k = assign_key(row[t]);
              if (k < best) { best = k; bt = t; }
            }
        }
        for (int o = g >> 1; o > 0; o >>= 1) {
          const unsigned long long ok = __shfl_xor(best, o, g);
          const int ot = __shfl_xor(bt, o, g);
          if (ok < best || (ok == best && ot < bt)) { best = ok; bt = ot; }
        }
        if (b >= 0 && gl == 0) rowinfo[b] = best == kAssignNoKey ? -3 : (pass << 10) | bt;
      }
      __syncthreads();
      // D
      bool took = false;
      if (mb >= 0 && rowinfo[mb] == ((pass << 10) | tid)) {
        freeb[mb] = 0;
        avail[tid] = 0;
        took = true;
      }
      if (tid == 0) nlist = 0;
      const int tk = __syncthreads_count(took);
      taken_in_pass += tk; navail -= tk; nfree -= tk;
      if (tk == 0 || navail == 0 || nfree == 0) break;
    }
    if (taken_in_pass == 0 || nfree == 0) break;
    pass++;
    if (tid < T) avail[tid] = 1;
    __syncthreads();
  }
  for (int b = tid; b < B; b += kAssignThreads) {
    const bool taken = !freeb[b];
    assign[b] = taken ? rowinfo[b] & 1023 : -1;
    if (pass_out) pass_out[b] = taken ? rowinfo[b] >> 10 : -1;
  }
}

}  // namespace rmpc
