// rmpc_timed.hpp -- conflict-free timed routes for a fleet, included by rmpc_world.hip: prioritised
// space-time planning on the grid (cooperative A*, Silver 2005, as a layered reachability sweep), several priority orders
// at once, and the follower that keeps the plan's order (Ma, Kumar, Koenig 2017).  The rules are written out in
// include/rmpc.h (rmpc_timed_plan_device, rmpc_timed_follow_device); everything is integer work on cells except the
// ranking of the end cells, which compares the doubles of a cost-to-go field as written.
//
// This header also holds the one copy of what the three space-time planners share (k_timed_plan here,
// k_timed_tours_plan in rmpc_timed_tours.hpp, k_timed_tours_replan in rmpc_timed_replan.hpp): the order check, the
// workspace of an order, the bit-row packer, the route of one robot through its stops (timed_robot) and the key; and of
// what the two followers and the two best-order kernels share.  The planners differ in where their inputs and outputs
// live, which stays in the kernels, and in the start rule, which is the template parameter of timed_robot: the
// later-starts rule (TimedLaterStarts, here) or the standing rule (TimedStandingRule, rmpc_timed_replan.hpp).
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

// the map, the rules' numbers and the thread's place in its workgroup: what every part of a plan is handed
struct TimedDims {
  int H, W, Wd, L, T, lag, sep2, rad, movement, tid, nt;
};

// the workspace of one order
struct TimedWork {
  timed_word *res, *hist, *freeb;    // the reservation table, the history (in LDS with kLds), the free mask
  timed_word *mask;                  // the start rule's mask of closed cells
  int *cnt;                          // the later-starts rule's counter per cell
};

template <bool kLds>
__device__ __forceinline__ TimedWork timed_work_at(timed_word *work, int g, const TimedGeom &q, int T) {
  extern __shared__ timed_word timed_lds[];
  TimedWork wk;
  wk.res = work + (size_t)g * q.per_order;
  wk.hist = kLds ? timed_lds : wk.res + (size_t)(T + 1) * q.L;
  wk.freeb = wk.res + 2 * (size_t)(T + 1) * q.L;
  wk.mask = wk.freeb + q.L;
  wk.cnt = (int *)(wk.mask + q.L);
  return wk;
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

// Every part of a plan below is called by the whole workgroup under uniform control flow.

// words[w] = the cells c of the map with in(c), as bit rows; `in` is resolved at compile time and may keep a state
template <class In>
__device__ __forceinline__ void timed_pack_rows(timed_word *__restrict__ words, const TimedDims &d, In &&in) {
  for (int w = d.tid; w < d.L; w += d.nt) {
    const int r = w / d.Wd, c0 = (w - r * d.Wd) * 64;
    timed_word word = 0;
    for (int bb = 0; bb < 64 && c0 + bb < d.W; bb++)
      if (in(r * d.W + c0 + bb)) word |= 1ull << bb;
    words[w] = word;
  }
}

// the cells that are not occupied
__device__ __forceinline__ void timed_free_mask(timed_word *__restrict__ freeb, const double *__restrict__ grid,
                                                double occ_threshold, const TimedDims &d) {
#pragma clang fp contract(off)
  timed_pack_rows(freeb, d, [=](int c) { return !(grid[c] >= occ_threshold); });
}

// whether the row of an order is no permutation of 0 .. B - 1 (the same answer in every thread)
__device__ __forceinline__ bool timed_order_bad(const int *__restrict__ ord, int B, int tid, int nt) {
  __shared__ unsigned seen[RMPC_TIMED_MAX_ROBOTS / 32];
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
  return __syncthreads_or(bad);
}

// the outputs of one order; the tours' rows are there with kServe (rmpc_timed_tours.hpp)
struct TimedOut {
  int *status, *arrive, *paths;      // [B], [B], [B][T + 1]
  int64_t *key;                      // the order's
  int *served, *serve_at, *unserved; // [B], [B][K], the order's
};

// what an order that is no permutation reports
template <bool kServe>
__device__ __forceinline__ void timed_bad_order(const TimedOut &o, int B, int T, int K, int tid, int nt) {
  for (int k = tid; k < B; k += nt) {
    o.status[k] = RMPC_TIMED_BAD_ORDER; o.arrive[k] = T + 1;
    if (kServe) o.served[k] = 0;
  }
  for (size_t i = tid; i < (size_t)B * (T + 1); i += nt) o.paths[i] = -1;
  if (kServe)
    for (size_t i = tid; i < (size_t)B * K; i += nt) o.serve_at[i] = -1;
  if (tid == 0) {
    *o.key = INT64_MAX;
    if (kServe) *o.unserved = INT_MAX;
  }
}

// thread 0's sums over the robots of one order
struct TimedKey {
  long long fails = 0, late = 0, sum = 0, uns = 0;
  // a robot that rule 1 skips, with n stops in a row of K
  __device__ __forceinline__ void skipped(int T, int n, int K) { late++; sum += T + 1; uns += n >= 0 && n <= K ? n : 0; }
  // a planned robot: status f, arrival layer a, done of n stops served
  __device__ __forceinline__ void planned(int f, int a, int T, int n, int done) {
    fails += f > 0; late += a > T; sum += a; uns += n - done;
  }
  __device__ __forceinline__ int64_t key() const { return (int64_t)((fails << 44) | (late << 32) | sum); }
};

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

// A start rule says which cells are closed to a robot in its early layers and until when a stop may not be held, in
// three operations: prepare(b, s) before robot b is planned from cell s; early(t), whether the rule's mask binds in
// layer t (uniform; on return the mask is the one of layer t); closed_until(sc, sw, sbit), the last layer in which cell
// sc (bit sbit of word sw) may not be held, -1 when it may be held in every layer.

// The later-starts rule: while t <= lag a robot keeps off the cells that conflict with the start of a robot ranked behind
// it.  cnt[c] = the robots not yet planned (and not skipped) whose start conflicts with c.
struct TimedLaterStarts {
  TimedDims d;
  int *cnt;
  timed_word *later;                 // the cells with cnt > 0

  // counts the starts of every robot of the order that skipped(b) does not leave out; ends behind a barrier
  template <class Skipped>
  __device__ __forceinline__ void count(const int *__restrict__ ord, const int *__restrict__ start_cell, int B, Skipped &&skipped) {
    for (int c = d.tid; c < d.H * d.W; c += d.nt) cnt[c] = 0;
    __syncthreads();
    for (int k = 0; k < B; k++) {
      const int b = ord[k];
      if (skipped(b)) continue;
      const int s = start_cell[b];
      timed_disc_count(cnt, d.H, d.W, s / d.W, s % d.W, d.rad, d.sep2, 1, d.tid, d.nt);
      __syncthreads();
    }
  }
  // (the barrier behind the first seed layer covers the mask)
  __device__ __forceinline__ void prepare(int, int s) {
    const int sr = s / d.W;
    timed_disc_count(cnt, d.H, d.W, sr, s - sr * d.W, d.rad, d.sep2, -1, d.tid, d.nt);
    __syncthreads();
    const int *const n = cnt;
    timed_pack_rows(later, d, [=](int c) { return n[c] > 0; });
  }
  __device__ __forceinline__ bool early(int t) const { return t <= d.lag; }
  __device__ __forceinline__ int closed_until(int, int sw, timed_word sbit) const { return later[sw] & sbit ? d.lag : -1; }
};

// how a robot's route ended: its status, its arrival layer (thread 0's) and the stops it served
struct TimedEnd {
  int f, a, done;
};

// The route of one robot from cell s at layer begin through its n stops (legs 0 .. n - 1, each a sweep that ends at the
// first layer in which the stop is reached and can be held for dwell layers) and on to the cell nearest its parking goal
// (leg n): path, status and arrive, then the path stamped into res.  Without kStops there are no stops (n is not read):
// the parking leg alone.  serve_at [n] takes the layers at which the stops are reached.  Without kStamp nothing is stamped
// (rmpc_cbs.hpp: a route under a table of constraints).  Ends behind a barrier.
template <bool kStops, bool kStamp = true, class Rule>
__device__ __forceinline__ TimedEnd timed_robot(const TimedDims &d, const TimedWork &wk, Rule &rule, const double *__restrict__ fields,
                                                const int *__restrict__ goal_cells, int s, int begin, int n_stops,
                                                const int *__restrict__ stops, int park, int dwell, int *__restrict__ path,
                                                int *__restrict__ serve_at, int *status, int *arrive, double *red_d,
                                                int *red_c) {
#pragma clang fp contract(off)
  const int H = d.H, W = d.W, HW = H * W, Wd = d.Wd, L = d.L, T = d.T, tid = d.tid, nt = d.nt;
  const int n = kStops ? n_stops : 0;
  timed_word *const hist = wk.hist, *const res = wk.res;
  for (int t = tid; t < begin; t += nt) path[t] = s;

  int t0 = begin, at = s, done = 0;  // the state; done: stops served
  int f = 0, te = 0, end = 0;        // how the last leg ended
  bool failed = false;
  for (int j = 0; j <= n && !failed; j++) {              // leg n is the parking leg (rule 4)
    const bool parking = !kStops || j == n;
    const int gi = parking ? park : stops[j];
    const int sc = parking ? -1 : goal_cells[gi];
    const bool inside = sc >= 0 && sc < HW;              // a stop outside the map is in no layer
    const int sw = inside ? (sc / W) * Wd + ((sc % W) >> 6) : 0;
    const timed_word sbit = inside ? 1ull << ((sc % W) & 63) : 0ull;
    timed_seed_layer(hist + (size_t)t0 * L, Wd, L, at / W, at % W, tid, nt);
    __syncthreads();
    int a = -1;
    f = 0;
    for (int t = t0;;) {                                 // at most T - t0 layers; the stop is tested in layer t0 too
      if (!parking && t + dwell <= T && (hist[(size_t)t * L + sw] & sbit)) {
        bool held = true;
        const int until = rule.closed_until(sc, sw, sbit);
        for (int u = t + 1; u <= t + dwell && held; u++) {
          if (__hip_atomic_load(res + (size_t)u * L + sw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & sbit) held = false;
          if (u <= until) held = false;
        }
        if (held) { a = t; break; }
      }
      if (++t > T) break;
      const bool early = rule.early(t);
      const bool any = timed_sweep_layer(hist + (size_t)(t - 1) * L, hist + (size_t)t * L, res + (size_t)t * L, wk.freeb,
                                         wk.mask, early, H, Wd, L, d.movement, tid, nt);
      if (!__syncthreads_or(any)) { f = t; break; }
    }
    if (a < 0) {
      // rules 3 and 4: the robot goes as near the leg's goal as it got and stays
      te = f ? f - 1 : T;
      end = timed_end_cell(fields + (size_t)gi * HW, hist + (size_t)te * L, W, Wd, L, red_d, red_c, tid, nt);
      failed = !parking;
      break;
    }
    for (int u = a + tid; u <= a + dwell; u += nt) path[u] = sc;
    if (tid == 0) {
      timed_backtrack(hist, L, H, W, Wd, d.movement, path, sc, a, t0);
      serve_at[j] = a;
    }
    t0 = a + dwell; at = sc; done++;
    __syncthreads();                                     // the backtrack has read the layers the next leg overwrites
  }
  for (int t = te + tid; t <= T; t += nt) path[t] = end;
  int a = T + 1;
  if (tid == 0) {
    timed_backtrack(hist, L, H, W, Wd, d.movement, path, end, te, t0);
    if (!failed && end == goal_cells[park]) {
      a = te;
      while (a > t0 && path[a - 1] == end) a--;
    }
    *status = f; *arrive = a;
  }
  __syncthreads();
  if (kStamp) {
    timed_stamp(res, path, H, W, Wd, L, T, d.lag, d.rad, d.sep2, tid, nt);
    __syncthreads();
  }
  return {f, a, done};
}

// One workgroup per priority order, its robots in rank order.  res is written with atomic ORs (the discs of different
// layers of a path overlap) and read with atomic loads, so that no reader is served a line from before the ORs.
template <bool kLds>
__global__ __launch_bounds__(kTimedThreads) void k_timed_plan(rmpc_timed_plan p, TimedGeom q, timed_word *__restrict__ work) {
  __shared__ double red_d[kTimedThreads];
  __shared__ int red_c[kTimedThreads];
  const int g = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, B = p.B, T = p.T, HW = p.H * p.W;
  const TimedDims d = {p.H, p.W, q.Wd, q.L, T, p.lag, p.sep2, q.rad, p.movement, tid, nt};
  const int *const ord = p.orders + (size_t)g * B;
  const TimedOut o = {p.status + (size_t)g * B, p.arrive + (size_t)g * B, p.paths + (size_t)g * B * (T + 1), p.key + g,
                      nullptr, nullptr, nullptr};
  if (timed_order_bad(ord, B, tid, nt)) {
    timed_bad_order<false>(o, B, T, 0, tid, nt);
    return;
  }

  const TimedWork wk = timed_work_at<kLds>(work, g, q, T);
  for (size_t i = tid; i < (size_t)(T + 1) * d.L; i += nt) wk.res[i] = 0;
  timed_free_mask(wk.freeb, p.grid, p.occ_threshold, d);
  const auto skipped = [&](int b) {
    const int s = p.start_cell[b], gi = p.goal_index[b];
    return s < 0 || s >= HW || gi < 0 || gi >= p.Gf;
  };
  TimedLaterStarts rule = {d, wk.cnt, wk.mask};
  rule.count(ord, p.start_cell, B, skipped);

  TimedKey key;
  for (int k = 0; k < B; k++) {
    const int b = ord[k];
    int *const path = o.paths + (size_t)b * (T + 1);
    if (skipped(b)) {
      for (int t = tid; t <= T; t += nt) path[t] = -1;
      if (tid == 0) { o.status[b] = RMPC_GRID_OUTSIDE; o.arrive[b] = T + 1; key.skipped(T, 0, 0); }
      continue;
    }
    const int s = p.start_cell[b];
    rule.prepare(b, s);
    const TimedEnd e = timed_robot<false>(d, wk, rule, p.fields, p.goal_cells, s, 0, 0, nullptr, p.goal_index[b], 0, path,
                                          nullptr, o.status + b, o.arrive + b, red_d, red_c);
    if (tid == 0) key.planned(e.f, e.a, T, 0, 0);
  }
  if (tid == 0) *o.key = key.key();
}

// the order with the least (unserved, key, g) among the valid ones (a valid key is below INT64_MAX), -1 when there is
// none; without kUnserved the least (key, g), and unserved and ru are not touched
template <bool kUnserved>
__device__ __forceinline__ void timed_best_order(const int64_t *__restrict__ key, const int *__restrict__ unserved, int G,
                                                 int *__restrict__ best, long long *rk, int *ru, int *rg) {
  const int tid = threadIdx.x;
  long long bk = INT64_MAX;
  int bu = INT_MAX, bg = -1;
  for (int g = tid; g < G; g += 256) {
    const long long k = key[g];
    const int u = kUnserved ? unserved[g] : 0;
    if (k < INT64_MAX && (bg < 0 || u < bu || (u == bu && k < bk))) { bu = u; bk = k; bg = g; }     // (g ascends)
  }
  rk[tid] = bk; rg[tid] = bg;
  if (kUnserved) ru[tid] = bu;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      const long long k = rk[tid + h];
      const int u = kUnserved ? ru[tid + h] : 0, mine = kUnserved ? ru[tid] : 0, g2 = rg[tid + h];
      if (g2 >= 0 && (rg[tid] < 0 || u < mine || (u == mine && (k < rk[tid] || (k == rk[tid] && g2 < rg[tid]))))) {
        rk[tid] = k; rg[tid] = g2;
        if (kUnserved) ru[tid] = u;
      }
    }
    __syncthreads();
  }
  if (tid == 0) *best = rg[0];
}

__global__ __launch_bounds__(256) void k_timed_best(const int64_t *__restrict__ key, int G, int *__restrict__ best) {
  __shared__ long long rk[256];
  __shared__ int rg[256];
  timed_best_order<false>(key, nullptr, G, best, rk, nullptr, rg);
}

// The followers' three steps; one workgroup per robot b, p its path.

// the index clamped into the path, and how far the robot is from that waypoint
__device__ __forceinline__ double timed_waypoint_dist(const int *__restrict__ p, int T, int &i, const double *__restrict__ pos_b,
                                                      int W, double x0, double y0, double cell) {
#pragma clang fp contract(off)
  i = i < 0 ? 0 : (i > T ? T : i);
  const int c = p[i];
  const double dx = (x0 + (double)(c % W) * cell) - pos_b[0];
  const double dy = (y0 + (double)(c / W) * cell) - pos_b[1];
  return sqrt(dx * dx + dy * dy);
}

// the least robot whose path can still block the step to p[i + 1], INT_MAX without one: the threads stride over the other
// robots j, each over the few layers s of j's path with idx_in[j] < s + lag <= i
__device__ __forceinline__ int timed_blocker(const int *__restrict__ paths, int B, int T, const int *__restrict__ idx_in, int b,
                                             const int *__restrict__ p, int i, int W, int sep2, int lag, int *red) {
  const int tid = threadIdx.x;
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
  return red[0];
}

// (one thread) the index, the goal at its waypoint and who blocks the robot
__device__ __forceinline__ void timed_goal_write(const int *__restrict__ p, int i, int blk, int b, int *__restrict__ idx_out,
                                                 double *__restrict__ goal, int *__restrict__ blocked, int W, double x0,
                                                 double y0, double cell) {
#pragma clang fp contract(off)
  const int cn = p[i];
  idx_out[b] = i;
  goal[(size_t)b * 3] = x0 + (double)(cn % W) * cell;
  goal[(size_t)b * 3 + 1] = y0 + (double)(cn / W) * cell;
  goal[(size_t)b * 3 + 2] = 0.0;
  if (blocked) blocked[b] = blk == INT_MAX ? -1 : blk;
}

// A robot that is not near its waypoint leaves at once.
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
  const double dist = timed_waypoint_dist(p, T, i, pos + (size_t)b * stride, W, x0, y0, cell);
  int blk = INT_MAX;
  bool advance = false;
  if (i < T && dist <= threshold) {       // (uniform over the workgroup)
    blk = timed_blocker(paths, B, T, idx_in, b, p, i, W, sep2, lag, red);
    advance = blk == INT_MAX;
  }
  if (tid == 0) timed_goal_write(p, advance ? i + 1 : i, blk, b, idx_out, goal, blocked, W, x0, y0, cell);
}

}  // namespace rmpc
