// rmpc_timed.hpp -- conflict-free timed routes for a fleet, included by rmpc_world.hip: prioritised
// space-time planning on the grid (cooperative A*, Silver 2005, as a layered reachability sweep), several priority orders
// at once, and the follower that keeps the plan's order (Ma, Kumar, Koenig 2017).  The rules are written out in
// include/rmpc.h (rmpc_timed_plan_device, rmpc_timed_follow_device); everything is integer work on cells except the
// ranking of the end cells, which compares the doubles of a cost-to-go field as written.
//
// A set of cells is held as bit rows: Wd = ceil(W / 64) words of 64 bits per row, bit (col & 63) of word
// row * Wd + col / 64; a layer has L = H Wd words.  Bits past column W - 1 are never set (the free mask clears them).
// One step of the reachability is then a few word operations per word: the word itself and the rows above and below
// (wait, row moves), their shifts by one column with the carry of the neighbouring words (column and diagonal moves),
// and with free & ~res[t].

#include <climits>
#include <cstdint>

namespace rmpc {

constexpr int kTimedThreads = 256;                // most threads of a workgroup: one word of a layer each per pass
constexpr int kTimedHistLds = 60 * 1024;          // the history of T + 1 layers lives in LDS up to this size (the
                                                  // store's 41 x 41 at T = 128: 42 KB), in the workspace beyond it
typedef unsigned long long timed_word;

struct TimedGeom {
  int Wd, L;                 // words per row, words per layer
  int rad;                   // the largest r with r * r < sep2: a disc's rows and columns reach this far
  long long per_order;       // words of workspace per order
};

// words of workspace of one order: res and the history ((T + 1) layers each), the free mask, the mask of the
// later-ranked starts, and one int32 counter per cell
static inline long long timed_order_words(int H, int W, int T) {
  const long long L = (long long)H * ((W + 63) / 64);
  return 2 * (long long)(T + 1) * L + 2 * L + ((long long)H * W + 1) / 2;
}

__device__ __forceinline__ bool timed_bit(const timed_word *layer, int Wd, int r, int col) {
  return (layer[r * Wd + (col >> 6)] >> (col & 63)) & 1ull;
}

// columns within h of col on row dr of a disc: the largest h with dr^2 + h^2 < sep2 (|dr| <= rad, so h >= 0)
__device__ __forceinline__ int timed_half_width(int dr, int rad, int sep2) {
  int h = rad;
  while (dr * dr + h * h >= sep2) h--;
  return h;
}

// cnt[c] += add on the cells that conflict with cell (r0, c0); the cells of one disc are distinct: no atomics
__device__ __forceinline__ void timed_disc_count(int *__restrict__ cnt, int H, int W, int r0, int c0, int rad, int sep2,
                                                 int add, int tid, int nt) {
  const int side = 2 * rad + 1;
  for (int i = tid; i < side * side; i += nt) {
    const int dr = i / side - rad, dc = i - (i / side) * side - rad;
    const int rr = r0 + dr, cc = c0 + dc;
    if (dr * dr + dc * dc < sep2 && rr >= 0 && rr < H && cc >= 0 && cc < W) cnt[rr * W + cc] += add;
  }
}

// The four parts of a robot's plan, shared by k_timed_plan and k_timed_tours_plan (rmpc_timed_tours.hpp).  Every one is
// called by the whole workgroup under uniform control flow.

// later[w] = the cells with cnt > 0: those that conflict with the start of a robot not yet planned
__device__ __forceinline__ void timed_later_mask(const int *__restrict__ cnt, timed_word *__restrict__ later, int W, int Wd,
                                                 int L, int tid, int nt) {
  for (int w = tid; w < L; w += nt) {
    const int r = w / Wd, c0 = (w - r * Wd) * 64;
    timed_word word = 0;
    for (int bb = 0; bb < 64 && c0 + bb < W; bb++)
      if (cnt[r * W + c0 + bb] > 0) word |= 1ull << bb;
    later[w] = word;
  }
}

// layer t of the history = {cell (sr, sc)}: where a robot stands when a sweep begins
__device__ __forceinline__ void timed_seed_layer(timed_word *__restrict__ layer, int Wd, int L, int sr, int sc, int tid, int nt) {
  for (int w = tid; w < L; w += nt) layer[w] = w == sr * Wd + (sc >> 6) ? 1ull << (sc & 63) : 0ull;
}

// reach[t] (cur) from reach[t - 1] (prev) and res[t] (rs); true when this thread wrote a word that is not empty.  The
// caller's __syncthreads_or is the layer's one barrier.
__device__ __forceinline__ bool timed_sweep_layer(const timed_word *prev, timed_word *cur, const timed_word *rs,
                                                  const timed_word *freeb, const timed_word *later, bool early, int H,
                                                  int Wd, int L, int movement, int tid, int nt) {
  bool any = false;
  for (int w = tid; w < L; w += nt) {
    const int r = Wd == 1 ? w : w / Wd, j = w - r * Wd;
    const bool up = r > 0, dn = r < H - 1;
    const timed_word P = prev[w];
    const timed_word V = P | (up ? prev[w - Wd] : 0ull) | (dn ? prev[w + Wd] : 0ull);
    timed_word S = P, Sl = 0, Sr = 0;         // what moves by one column: the row itself, with 8 moves its neighbours too
    if (j > 0) Sl = prev[w - 1];
    if (j < Wd - 1) Sr = prev[w + 1];
    if (movement == 8) {
      S = V;
      if (j > 0) Sl |= (up ? prev[w - 1 - Wd] : 0ull) | (dn ? prev[w - 1 + Wd] : 0ull);
      if (j < Wd - 1) Sr |= (up ? prev[w + 1 - Wd] : 0ull) | (dn ? prev[w + 1 + Wd] : 0ull);
    }
    timed_word n = V | (S << 1) | (Sl >> 63) | (S >> 1) | (Sr << 63);
    n &= freeb[w] & ~__hip_atomic_load(rs + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (early) n &= ~later[w];
    cur[w] = n;
    any = any || n != 0ull;
  }
  return any;
}

// the end cell: the least (F(c), c) over the layer E; an F that is not below +inf ranks as +inf.  nt is a power of two;
// ends behind a barrier, so every thread gets the cell (INT_MAX for an empty layer).
__device__ __forceinline__ int timed_end_cell(const double *__restrict__ F, const timed_word *E, int W, int Wd, int L,
                                              double *red_d, int *red_c, int tid, int nt) {
  double bd = __builtin_inf();
  int bc = INT_MAX;
  for (int w = tid; w < L; w += nt) {
    const int r = w / Wd, c0 = r * W + (w - r * Wd) * 64;
    timed_word word = E[w];
    while (word) {
      const int c = c0 + __ffsll((long long)word) - 1;
      word &= word - 1;
      double d = F[c];
      d = d < __builtin_inf() ? d : __builtin_inf();
      if (d < bd || (d == bd && c < bc)) { bd = d; bc = c; }
    }
  }
  red_d[tid] = bd; red_c[tid] = bc;
  __syncthreads();
  for (int h = nt >> 1; h > 0; h >>= 1) {
    if (tid < h) {
      const double d = red_d[tid + h];
      const int c = red_c[tid + h];
      if (d < red_d[tid] || (d == red_d[tid] && c < red_c[tid])) { red_d[tid] = d; red_c[tid] = c; }
    }
    __syncthreads();
  }
  return red_c[0];
}

// backwards from (te, c) down to layer t0 (one thread): path[t - 1] for t = te .. t0 + 1, wait first, else the first move
// in move order whose origin was reachable
__device__ __forceinline__ void timed_backtrack(const timed_word *hist, int L, int H, int W, int Wd, int movement,
                                                int *__restrict__ path, int c, int te, int t0) {
  for (int t = te; t > t0; t--) {
    const timed_word *const prev = hist + (size_t)(t - 1) * L;
    const int r = c / W, col = c - r * W;
    if (!timed_bit(prev, Wd, r, col)) {
      for (int m = 0; m < movement; m++) {
        const int rr = r - grid_dr(m), cc = col - grid_dc(m);
        if (rr >= 0 && rr < H && cc >= 0 && cc < W && timed_bit(prev, Wd, rr, cc)) { c = rr * W + cc; break; }
      }
    }
    path[t - 1] = c;
  }
}

// stamping: the cells that conflict with path[t] into res[s], |s - t| <= lag, one (t, disc row, s) per thread and pass;
// with kOnMap a path[t] outside [0, H W) stamps nothing (the plans' own paths never hold one)
template <bool kOnMap = false>
__device__ __forceinline__ void timed_stamp(timed_word *res, const int *__restrict__ path, int H, int W, int Wd, int L, int T,
                                            int lag, int rad, int sep2, int tid, int nt) {
  const int side = 2 * rad + 1, nl = 2 * lag + 1;
  const long long total = (long long)(T + 1) * side * nl;
  for (long long i = tid; i < total; i += nt) {
    const int t = (int)(i / (side * nl)), rem = (int)(i - (long long)t * side * nl);
    const int dr = rem / nl - rad, sl = t - lag + (rem - (rem / nl) * nl);
    if (sl < 0 || sl > T) continue;
    const int c = path[t], r = c / W + dr, col = c % W;
    if (kOnMap && (c < 0 || c >= H * W)) continue;
    if (r < 0 || r >= H) continue;
    const int h = timed_half_width(dr, rad, sep2);
    const int lo = col - h > 0 ? col - h : 0, hi = col + h < W - 1 ? col + h : W - 1;
    for (int j = lo >> 6; j <= hi >> 6; j++) {
      const int a = (lo > j * 64 ? lo : j * 64) - j * 64, e = (hi < j * 64 + 63 ? hi : j * 64 + 63) - j * 64;
      const timed_word mask = (e == 63 ? ~0ull : (1ull << (e + 1)) - 1ull) & ~((1ull << a) - 1ull);
      __hip_atomic_fetch_or(res + (size_t)sl * L + r * Wd + j, mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// One workgroup per priority order, its robots in rank order.  res is written with atomic ORs (the discs of different
// layers of a path overlap) and read with atomic loads, so that no reader is served a line from before the ORs.
template <bool kLds>
__global__ __launch_bounds__(kTimedThreads) void k_timed_plan(rmpc_timed_plan p, TimedGeom q, timed_word *__restrict__ work) {
#pragma clang fp contract(off)
  extern __shared__ timed_word timed_lds[];
  __shared__ unsigned seen[RMPC_TIMED_MAX_ROBOTS / 32];
  __shared__ double red_d[kTimedThreads];
  __shared__ int red_c[kTimedThreads];
  const int g = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int H = p.H, W = p.W, HW = H * W, B = p.B, T = p.T, Wd = q.Wd, L = q.L, lag = p.lag, sep2 = p.sep2, rad = q.rad;
  const int *const ord = p.orders + (size_t)g * B;
  int *const status = p.status + (size_t)g * B, *const arrive = p.arrive + (size_t)g * B;
  int *const paths = p.paths + (size_t)g * B * (T + 1);

  // the order must be a permutation of 0 .. B - 1
  for (int i = tid; i < RMPC_TIMED_MAX_ROBOTS / 32; i += nt) seen[i] = 0;
  __syncthreads();
  bool bad = false;
  for (int k = tid; k < B; k += nt) {
    const int v = ord[k];
    if (v < 0 || v >= B) bad = true;
    else {
      const unsigned bit = 1u << (v & 31);
      if (atomicOr(&seen[v >> 5], bit) & bit) bad = true;
    }
  }
  if (__syncthreads_or(bad)) {
    for (int k = tid; k < B; k += nt) { status[k] = RMPC_TIMED_BAD_ORDER; arrive[k] = T + 1; }
    for (size_t i = tid; i < (size_t)B * (T + 1); i += nt) paths[i] = -1;
    if (tid == 0) p.key[g] = INT64_MAX;
    return;
  }

  timed_word *const res = work + (size_t)g * q.per_order;
  timed_word *const hist = kLds ? timed_lds : res + (size_t)(T + 1) * L;
  timed_word *const freeb = res + 2 * (size_t)(T + 1) * L;
  timed_word *const later = freeb + L;
  int *const cnt = (int *)(later + L);

  for (size_t i = tid; i < (size_t)(T + 1) * L; i += nt) res[i] = 0;
  for (int w = tid; w < L; w += nt) {
    const int r = w / Wd, c0 = (w - r * Wd) * 64;
    timed_word word = 0;
    for (int b = 0; b < 64 && c0 + b < W; b++)
      if (!(p.grid[r * W + c0 + b] >= p.occ_threshold)) word |= 1ull << b;
    freeb[w] = word;
  }
  for (int c = tid; c < HW; c += nt) cnt[c] = 0;
  __syncthreads();
  // cnt[c] = the robots not yet planned (and not skipped) whose start conflicts with c
  for (int k = 0; k < B; k++) {
    const int b = ord[k], s = p.start_cell[b], gi = p.goal_index[b];
    if (s < 0 || s >= HW || gi < 0 || gi >= p.Gf) continue;
    timed_disc_count(cnt, H, W, s / W, s % W, rad, sep2, 1, tid, nt);
    __syncthreads();
  }

  long long fails = 0, late = 0, sum = 0;       // (thread 0's)
  for (int k = 0; k < B; k++) {
    const int b = ord[k], s = p.start_cell[b], gi = p.goal_index[b];
    int *const path = paths + (size_t)b * (T + 1);
    if (s < 0 || s >= HW || gi < 0 || gi >= p.Gf) {
      for (int t = tid; t <= T; t += nt) path[t] = -1;
      if (tid == 0) { status[b] = RMPC_GRID_OUTSIDE; arrive[b] = T + 1; late++; sum += T + 1; }
      continue;
    }
    const int sr = s / W, sc = s - sr * W;
    timed_disc_count(cnt, H, W, sr, sc, rad, sep2, -1, tid, nt);
    __syncthreads();
    timed_later_mask(cnt, later, W, Wd, L, tid, nt);
    timed_seed_layer(hist, Wd, L, sr, sc, tid, nt);
    __syncthreads();

    // the layers: reach[t] from reach[t - 1]; one barrier per layer, which also tells whether the layer is empty
    int f = 0;
    for (int t = 1; t <= T; t++) {
      const bool any = timed_sweep_layer(hist + (size_t)(t - 1) * L, hist + (size_t)t * L, res + (size_t)t * L, freeb, later,
                                         t <= lag, H, Wd, L, p.movement, tid, nt);
      if (!__syncthreads_or(any)) { f = t; break; }
    }
    const int te = f ? f - 1 : T;

    // the end cell: the least (D_goal(c), c) over reach[te]
    const int end = timed_end_cell(p.fields + (size_t)gi * HW, hist + (size_t)te * L, W, Wd, L, red_d, red_c, tid, nt);
    for (int t = te + tid; t <= T; t += nt) path[t] = end;
    if (tid == 0) {
      timed_backtrack(hist, L, H, W, Wd, p.movement, path, end, te, 0);
      int a = T + 1;
      if (end == p.goal_cells[gi]) {
        a = te;
        while (a > 0 && path[a - 1] == end) a--;
      }
      status[b] = f; arrive[b] = a;
      fails += f > 0; late += a > T; sum += a;
    }
    __syncthreads();
    timed_stamp(res, path, H, W, Wd, L, T, lag, rad, sep2, tid, nt);
    __syncthreads();
  }
  if (tid == 0) p.key[g] = (int64_t)((fails << 44) | (late << 32) | sum);
}

// the order with the least (key, g) among the valid ones (a valid key is below INT64_MAX), -1 when there is none
__global__ __launch_bounds__(256) void k_timed_best(const int64_t *__restrict__ key, int G, int *__restrict__ best) {
  __shared__ long long rk[256];
  __shared__ int rg[256];
  const int tid = threadIdx.x;
  long long bk = INT64_MAX;
  int bg = -1;
  for (int g = tid; g < G; g += 256) {
    const long long k = key[g];
    if (k < bk) { bk = k; bg = g; }            // (g ascends: the lower g wins ties)
  }
  rk[tid] = bk; rg[tid] = bg;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      const long long k = rk[tid + h];
      const int g2 = rg[tid + h];
      if (g2 >= 0 && (k < rk[tid] || (k == rk[tid] && (rg[tid] < 0 || g2 < rg[tid])))) { rk[tid] = k; rg[tid] = g2; }
    }
    __syncthreads();
  }
  if (tid == 0) *best = rg[0];
}

// One workgroup per robot; its threads stride over the other robots j, each over the few layers s of j's path that
// can still block: idx_in[j] < s + lag <= i.  A robot that is not near its waypoint leaves at once.
__global__ __launch_bounds__(256) void k_timed_follow(const int *__restrict__ paths, int B, int T, const int *__restrict__ idx_in,
                                                      int *__restrict__ idx_out, const double *__restrict__ pos, int stride,
                                                      int W, double x0, double y0, double cell, double threshold, int sep2,
                                                      int lag, double *__restrict__ goal, int *__restrict__ blocked) {
#pragma clang fp contract(off)
  __shared__ int red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int *const p = paths + (size_t)b * (T + 1);
  if (p[0] < 0) {
    if (tid == 0) { idx_out[b] = idx_in[b]; if (blocked) blocked[b] = -1; }
    return;
  }
  int i = idx_in[b];
  i = i < 0 ? 0 : (i > T ? T : i);
  const int c = p[i];
  const double dx = (x0 + (double)(c % W) * cell) - pos[(size_t)b * stride];
  const double dy = (y0 + (double)(c / W) * cell) - pos[(size_t)b * stride + 1];
  int blk = INT_MAX;
  bool advance = false;
  if (i < T && sqrt(dx * dx + dy * dy) <= threshold) {       // (uniform over the workgroup)
    const int qc = p[i + 1], qr = qc / W, qcol = qc % W;
    int mine = INT_MAX;
    for (int j = tid; j < B && mine == INT_MAX; j += 256) {
      if (j == b) continue;
      const int *const pj = paths + (size_t)j * (T + 1);
      if (pj[0] < 0) continue;
      const long long first = (long long)idx_in[j] - lag + 1;           // the least s with idx_in[j] < s + lag
      for (int s = first > 0 ? (int)first : 0; s <= i - lag; s++) {
        const int cj = pj[s], er = cj / W - qr, ec = cj % W - qcol;
        if ((long long)er * er + (long long)ec * ec < (long long)sep2) { mine = j; break; }
      }
    }
    red[tid] = mine;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h && red[tid + h] < red[tid]) red[tid] = red[tid + h];
      __syncthreads();
    }
    blk = red[0];
    advance = blk == INT_MAX;
  }
  if (tid == 0) {
    if (advance) i++;
    const int cn = p[i];
    idx_out[b] = i;
    goal[(size_t)b * 3] = x0 + (double)(cn % W) * cell;
    goal[(size_t)b * 3 + 1] = y0 + (double)(cn / W) * cell;
    goal[(size_t)b * 3 + 2] = 0.0;
    if (blocked) blocked[b] = blk == INT_MAX ? -1 : blk;
  }
}

}  // namespace rmpc
