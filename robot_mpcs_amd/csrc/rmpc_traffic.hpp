// rmpc_traffic.hpp -- traffic-aware routes (include/rmpc_traffic.h), included by rmpc_world.hip:
// k_traffic_add counts routes into the flow table, k_traffic_fields builds one cost-to-go field per goal whose edge
// costs read the table, k_traffic_paths walks such fields down to the goal, k_traffic_score reduces a table to
// (L, V, C).  The rule is the header's.  Everything is integer arithmetic: every update of a field is a monotone min
// from INF of the same expression, so any order of in-place updates reaches the same fixed point (the argument of
// rmpc_grid.hpp), bit for bit that of a plain restatement.  Every loop is bounded, no workgroup waits for another.

namespace rmpc {

constexpr int kTrafficInf = RMPC_TRAFFIC_INF;
constexpr int kTrafficScoreThreads = 1024;

struct TrafficCosts {                       // rmpc_traffic_costs, checked by the entry
  int base_axial, base_diag, w_visit, cap_visit, w_contra, cap_contra;
};

__device__ __forceinline__ int traffic_opp(int m) { return m ^ 2; }      // 0 <-> 2, 1 <-> 3, 4 <-> 6, 5 <-> 7
__device__ __forceinline__ int traffic_capped(int n, int cap) { return n < 0 ? 0 : (n > cap ? cap : n); }

// One thread per (robot, route cell): the visit of its cell, and the move to the next cell where there is one.
__global__ __launch_bounds__(256) void k_traffic_add(int H, int W, int B, const int *__restrict__ path,
                                                     const int *__restrict__ len, int max_len,
                                                     const int *__restrict__ select, int sign, int *__restrict__ flow) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * max_len) return;
  const int b = (int)(i / max_len), k = (int)(i - (long long)b * max_len), HW = H * W;
  const int n = len[b] < max_len ? len[b] : max_len;
  if (k >= n || (select && select[b] == 0)) return;
  const int u = path[i];
  if (u < 0 || u >= HW) return;
  atomicAdd(flow + (size_t)8 * HW + u, sign);
  if (k + 1 >= n) return;
  const int v = path[i + 1];
  if (v < 0 || v >= HW) return;
  const int dr = v / W - u / W, dc = v % W - u % W;
#pragma unroll
  for (int m = 0; m < 8; m++)
    if (dr == grid_dr(m) && dc == grid_dc(m)) atomicAdd(flow + (size_t)m * HW + u, sign);
}

// One workgroup per goal, the layout of k_grid_fields: thread t owns the cells t * per .. t * per + per - 1 (per odd,
// <= 17: the lanes of one LDS access are `per` words apart, every lane on its own bank).  LDS holds
// E(v) = w_visit * min(vis(v), cap_visit) + D(v) of every cell as one int32 (INF where D is INF), so a relaxation reads
// one word per neighbour.  The contraflow term belongs to the pair (u, m); it is kept at the owning cell u: eight 4-bit
// capped counts min(flow [opp(m)][u + m], cap_contra) in one word per cell (cap_contra <= 15), packed in the prologue
// and read once per relaxation.  These words live in LDS too, not in registers: the sweeps are unrolled over a thread's
// cells, the cost of every (cell, move) is invariant in the sweep loop, and with the words in registers the compiler
// hoists all 136 costs out of the loop and spills (368 bytes of scratch per lane); a load behind the sweep's barrier
// cannot be hoisted.  A cell's own capped visits, read only when its D drops, are a byte per cell in LDS.  The flags
// are those of k_grid_fields, 10 bits per cell and three cells to a register (bit m: u + m inside the map, bit 8: the
// cell takes part, free and not the goal).  64 + 64 + 16 KiB of LDS, one workgroup per CU as k_grid_fields has.
//
// Candidates are formed unsigned: E <= INF = 2^31 - 1 and an edge costs at most 65535, so E + cost never wraps, and a
// candidate made from INF stays above INF -- it loses every min without a test.  The weights fit 16 bits and the counts
// 8, so the products are 24-bit multiplies.
__global__ __launch_bounds__(kGridThreads) void k_traffic_fields(const double *__restrict__ grid, int H, int W,
                                                                 double occ_threshold, const int *__restrict__ flow,
                                                                 TrafficCosts k, const int *__restrict__ goal_cells,
                                                                 int nmoves, int *__restrict__ fields,
                                                                 int *__restrict__ status, int *__restrict__ sweeps) {
  __shared__ unsigned E[kGridMaxCells];
  __shared__ unsigned Contra[kGridMaxCells];
  __shared__ unsigned char Vis[kGridMaxCells];
  const int HW = H * W, g = blockIdx.x, t = threadIdx.x;
  const int per = ((HW + kGridThreads - 1) / kGridThreads) | 1;
  const int goal = goal_cells[g];
  const bool goal_in = goal >= 0 && goal < HW;
  const bool goal_ok = goal_in && grid[goal] < occ_threshold;
  int *const F = fields + (size_t)g * HW;
  const unsigned inf = (unsigned)kTrafficInf;
  if (!goal_ok) {
    for (int c = t; c < HW; c += kGridThreads) F[c] = kTrafficInf;
    if (t == 0) { status[g] = goal_in ? RMPC_GRID_GOAL_OCCUPIED : RMPC_GRID_OUTSIDE; if (sweeps) sweeps[g] = 0; }
    return;
  }
  const unsigned wv = (unsigned)k.w_visit, wc = (unsigned)k.w_contra;
  unsigned *const Et = E + t * per;
  unsigned D[kGridPer], fw[(kGridPer + 2) / 3];
#pragma unroll
  for (int w = 0; w < (kGridPer + 2) / 3; w++) fw[w] = 0;
#define RMPC_TRAFFIC_FLAGS(i) ((fw[(i) / 3] >> (10 * ((i) % 3))) & 1023u)
  // The prologue reads the table in a loop that stays rolled (few registers, little code); a cell's flags reach their
  // register through the cell's own word of E.
#pragma unroll 1
  for (int i = 0; i < per; i++) {
    const int c = t * per + i;
    if (c >= HW) break;
    const int r = c / W, col = c - r * W;
    unsigned f = 0, packed = 0;
#pragma unroll 1
    for (int m = 0; m < nmoves; m++) {
      const int rr = r + grid_dr(m), cc = col + grid_dc(m);
      if (rr >= 0 && rr < H && cc >= 0 && cc < W) {
        f |= 1u << m;
        packed |= (unsigned)traffic_capped(flow[(size_t)traffic_opp(m) * HW + rr * W + cc], k.cap_contra) << (4 * m);
      }
    }
    if (c != goal && grid[c] < occ_threshold) f |= 256u;
    Contra[c] = packed;
    Vis[c] = (unsigned char)traffic_capped(flow[(size_t)8 * HW + c], k.cap_visit);
    Et[i] = f;
  }
#pragma unroll
  for (int i = 0; i < kGridPer; i++) {
    const int c = t * per + i;
    const bool own = i < per && c < HW;
    if (own) fw[i / 3] |= Et[i] << (10 * (i % 3));
    D[i] = own && c == goal ? 0u : inf;
    if (own) Et[i] = c == goal ? __umul24(wv, Vis[c]) : inf;
  }
  __syncthreads();
  const unsigned char *const Vt = Vis + t * per;
  const unsigned *const Ct = Contra + t * per;
  auto relax = [&](int i, bool &lowered) {
    const unsigned flags = RMPC_TRAFFIC_FLAGS(i);
    if (flags & 256u) {
      unsigned best = D[i];
      const unsigned contra = Ct[i];
#pragma unroll
      for (int m = 0; m < 8; m++)
        if (flags & (1u << m)) {
          const unsigned base = (unsigned)(m < 4 ? k.base_axial : k.base_diag);
          const unsigned cand = Et[i + grid_dr(m) * W + grid_dc(m)] + (base + __umul24(wc, (contra >> (4 * m)) & 15u));
          best = cand < best ? cand : best;
        }
      if (best < D[i]) {
        D[i] = best;
        Et[i] = best + __umul24(wv, Vt[i]);
        lowered = true;
      }
    }
  };
  // Costs >= 1: every sweep does at least one Jacobi step, so a field is final after at most H W sweeps (the depth of
  // its shortest-path tree) plus the quiet one; the bound keeps the loop finite whatever the inputs hold.
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
    if (i < per && c < HW) F[c] = converged ? (int)D[i] : kTrafficInf;
  }
#undef RMPC_TRAFFIC_FLAGS
  if (t == 0) {
    status[g] = converged ? RMPC_GRID_OK : RMPC_GRID_NO_FIXED_POINT;
    if (sweeps) sweeps[g] = converged ? sweep + 1 : sweep;
  }
}

// descent of field goal_index [b] from start_cell [b]: the header's step rule, one thread per robot
__global__ __launch_bounds__(256) void k_traffic_paths(const double *__restrict__ grid, int H, int W, double occ_threshold,
                                                       const int *__restrict__ flow, TrafficCosts k,
                                                       const int *__restrict__ fields, const int *__restrict__ goal_cells,
                                                       int G, const int *__restrict__ start_cell,
                                                       const int *__restrict__ goal_index, int B, int nmoves, int max_len,
                                                       int *__restrict__ path, int *__restrict__ len) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int HW = H * W, s = start_cell[b], gi = goal_index[b];
  const int goal = gi >= 0 && gi < G ? goal_cells[gi] : -1;
  int *const out = path + (size_t)b * max_len;
  if (s < 0 || s >= HW || goal < 0 || goal >= HW) { len[b] = RMPC_GRID_OUTSIDE; return; }
  if (!(grid[s] < occ_threshold)) { len[b] = RMPC_GRID_START_OCCUPIED; return; }
  if (!(grid[goal] < occ_threshold)) { len[b] = RMPC_GRID_GOAL_OCCUPIED; return; }
  const int *const F = fields + (size_t)gi * HW;
  if (F[s] == kTrafficInf) { len[b] = 0; return; }
  int u = s, n = 0;
  for (;;) {
    if (n >= max_len) { len[b] = RMPC_GRID_TOO_LONG; return; }
    out[n++] = u;
    if (u == goal) break;
    const int r = u / W, col = u - r * W;
    int best = kTrafficInf, next = -1;
    for (int m = 0; m < nmoves; m++) {
      const int rr = r + grid_dr(m), cc = col + grid_dc(m);
      if (rr < 0 || rr >= H || cc < 0 || cc >= W) continue;
      const int v = rr * W + cc, Dv = F[v];
      if (Dv == kTrafficInf) continue;
      const int cand = (m < 4 ? k.base_axial : k.base_diag) + k.w_visit * traffic_capped(flow[(size_t)8 * HW + v], k.cap_visit) +
                       k.w_contra * traffic_capped(flow[(size_t)traffic_opp(m) * HW + v], k.cap_contra) + Dv;
      if (cand < best) { best = cand; next = v; }
    }
    if (next < 0) { len[b] = 0; return; }   // (not reached on a field of this grid and table)
    u = next;
  }
  len[b] = n;
}

// (L, V, C) of a table: one workgroup, every thread sums its cells t, t + 1024, ..., then a tree in LDS -- a fixed
// order, and integers besides
__global__ __launch_bounds__(kTrafficScoreThreads) void k_traffic_score(int H, int W, const int *__restrict__ flow,
                                                                        int base_axial, int base_diag,
                                                                        long long *__restrict__ score) {
  __shared__ long long acc[3][kTrafficScoreThreads];
  const int HW = H * W, t = threadIdx.x;
  long long L = 0, V = 0, Cf = 0;
  for (int c = t; c < HW; c += kTrafficScoreThreads) {
    const int r = c / W, col = c - r * W;
    for (int m = 0; m < 8; m++) {
      const long long f = flow[(size_t)m * HW + c];
      L += (long long)(m < 4 ? base_axial : base_diag) * f;
      if (m == 0 || m == 1 || m == 4 || m == 5) {        // one of each pair of opposite moves: every unordered pair once
        const int rr = r + grid_dr(m), cc = col + grid_dc(m);
        if (rr >= 0 && rr < H && cc >= 0 && cc < W) Cf += f * (long long)flow[(size_t)traffic_opp(m) * HW + rr * W + cc];
      }
    }
    const long long n = flow[(size_t)8 * HW + c];
    V += n * (n - 1) / 2;
  }
  acc[0][t] = L; acc[1][t] = V; acc[2][t] = Cf;
  __syncthreads();
  for (int s = kTrafficScoreThreads / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int j = 0; j < 3; j++) acc[j][t] += acc[j][t + s];
    __syncthreads();
  }
  if (t < 3) score[t] = acc[t][0];
}

}  // namespace rmpc
