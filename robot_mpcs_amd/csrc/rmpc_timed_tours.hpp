// rmpc_timed_tours.hpp -- timed tours (include/rmpc_timed_tours.h), included by rmpc_world.hip behind
// rmpc_timed.hpp, whose bit rows, layer sweep, end-cell reduction, backtrack and stamping it calls: the plan of
// rmpc_timed.hpp with a sequence of stops per robot, each leg a sweep that ends at the first layer in which the stop can
// be reached and held, and the follower with the serve step.  What is added to a layer is uniform over the workgroup:
// one bit test of the stop's cell, and up to `dwell` loads of res.

#include <climits>
#include <cstdint>

namespace rmpc {

// rule 1 of include/rmpc_timed_tours.h (every thread reads the same words)
__device__ __forceinline__ bool timed_tours_skipped(const rmpc_timed_tours &p, int b, int HW) {
  const int s = p.start_cell[b], n = p.len[b], pk = p.park_index[b];
  if (s < 0 || s >= HW || n < 0 || n > p.K || pk < 0 || pk >= p.Gf) return true;
  for (int j = 0; j < n; j++) {
    const int v = p.stops[(size_t)b * p.K + j];
    if (v < 0 || v >= p.Gf) return true;
  }
  return false;
}

// One workgroup per priority order, as k_timed_plan.  The history holds the layers of the current leg only: a leg writes
// the layers from its t0 on, and its backtrack is taken before the next leg begins.
template <bool kLds>
__global__ __launch_bounds__(kTimedThreads) void k_timed_tours_plan(rmpc_timed_tours p, TimedGeom q, timed_word *__restrict__ work) {
#pragma clang fp contract(off)
  extern __shared__ timed_word timed_lds[];
  __shared__ unsigned seen[RMPC_TIMED_MAX_ROBOTS / 32];
  __shared__ double red_d[kTimedThreads];
  __shared__ int red_c[kTimedThreads];
  const int g = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int H = p.H, W = p.W, HW = H * W, B = p.B, T = p.T, K = p.K, Wd = q.Wd, L = q.L, lag = p.lag, sep2 = p.sep2, rad = q.rad;
  const int dwell = p.dwell;
  const int *const ord = p.orders + (size_t)g * B;
  int *const status = p.status + (size_t)g * B, *const arrive = p.arrive + (size_t)g * B;
  int *const served = p.served + (size_t)g * B;
  int *const paths = p.paths + (size_t)g * B * (T + 1);
  int *const serve_at = p.serve_at + (size_t)g * B * K;

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
    for (int k = tid; k < B; k += nt) { status[k] = RMPC_TIMED_BAD_ORDER; arrive[k] = T + 1; served[k] = 0; }
    for (size_t i = tid; i < (size_t)B * (T + 1); i += nt) paths[i] = -1;
    for (size_t i = tid; i < (size_t)B * K; i += nt) serve_at[i] = -1;
    if (tid == 0) { p.key[g] = INT64_MAX; p.unserved[g] = INT_MAX; }
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
    const int b = ord[k];
    if (timed_tours_skipped(p, b, HW)) continue;
    const int s = p.start_cell[b];
    timed_disc_count(cnt, H, W, s / W, s % W, rad, sep2, 1, tid, nt);
    __syncthreads();
  }

  long long fails = 0, late = 0, sum = 0, uns = 0;       // (thread 0's)
  for (int k = 0; k < B; k++) {
    const int b = ord[k], n = p.len[b];
    int *const path = paths + (size_t)b * (T + 1);
    int *const sa = serve_at + (size_t)b * K;
    for (int j = tid; j < K; j += nt) sa[j] = -1;
    if (timed_tours_skipped(p, b, HW)) {
      for (int t = tid; t <= T; t += nt) path[t] = -1;
      if (tid == 0) {
        status[b] = RMPC_GRID_OUTSIDE; arrive[b] = T + 1; served[b] = 0;
        late++; sum += T + 1; uns += n >= 0 && n <= K ? n : 0;
      }
      continue;
    }
    const int s = p.start_cell[b];
    timed_disc_count(cnt, H, W, s / W, s - (s / W) * W, rad, sep2, -1, tid, nt);
    __syncthreads();
    timed_later_mask(cnt, later, W, Wd, L, tid, nt);      // (the seed's barrier below covers it)

    int t0 = 0, at = s, done = 0;      // the state; done: stops served
    int f = 0, te = 0, end = 0;        // how the last leg ended
    bool failed = false;
    for (int j = 0; j < n; j++) {
      const int gi = p.stops[(size_t)b * K + j], sc = p.goal_cells[gi];
      const bool inside = sc >= 0 && sc < HW;              // a stop outside the map is in no layer
      const int sw = inside ? (sc / W) * Wd + ((sc % W) >> 6) : 0;
      const timed_word sbit = inside ? 1ull << ((sc % W) & 63) : 0ull;
      timed_seed_layer(hist + (size_t)t0 * L, Wd, L, at / W, at % W, tid, nt);
      __syncthreads();
      int a = -1;
      f = 0;
      for (int t = t0; t <= T; t++) {                      // at most T - t0 layers
        if (t > t0) {
          const bool any = timed_sweep_layer(hist + (size_t)(t - 1) * L, hist + (size_t)t * L, res + (size_t)t * L, freeb,
                                             later, t <= lag, H, Wd, L, p.movement, tid, nt);
          if (!__syncthreads_or(any)) { f = t; break; }
        }
        if (t + dwell <= T && (hist[(size_t)t * L + sw] & sbit)) {
          bool held = true;
          for (int u = t + 1; u <= t + dwell && held; u++) {
            if (__hip_atomic_load(res + (size_t)u * L + sw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & sbit) held = false;
            if (u <= lag && (later[sw] & sbit)) held = false;
          }
          if (held) { a = t; break; }
        }
      }
      if (a < 0) {
        // rule 3: the robot goes as near the stop as it got and stays
        te = f ? f - 1 : T;
        end = timed_end_cell(p.fields + (size_t)gi * HW, hist + (size_t)te * L, W, Wd, L, red_d, red_c, tid, nt);
        failed = true;
        break;
      }
      for (int u = a + tid; u <= a + dwell; u += nt) path[u] = sc;
      if (tid == 0) {
        timed_backtrack(hist, L, H, W, Wd, p.movement, path, sc, a, t0);
        sa[j] = a;
      }
      t0 = a + dwell; at = sc; done++;
      __syncthreads();                                     // the backtrack has read the layers the next leg overwrites
    }
    if (!failed) {
      // rule 4: the parking leg
      timed_seed_layer(hist + (size_t)t0 * L, Wd, L, at / W, at % W, tid, nt);
      __syncthreads();
      f = 0;
      for (int t = t0 + 1; t <= T; t++) {
        const bool any = timed_sweep_layer(hist + (size_t)(t - 1) * L, hist + (size_t)t * L, res + (size_t)t * L, freeb, later,
                                           t <= lag, H, Wd, L, p.movement, tid, nt);
        if (!__syncthreads_or(any)) { f = t; break; }
      }
      te = f ? f - 1 : T;
      end = timed_end_cell(p.fields + (size_t)p.park_index[b] * HW, hist + (size_t)te * L, W, Wd, L, red_d, red_c, tid, nt);
    }
    for (int t = te + tid; t <= T; t += nt) path[t] = end;
    if (tid == 0) {
      timed_backtrack(hist, L, H, W, Wd, p.movement, path, end, te, t0);
      int a = T + 1;
      if (!failed && end == p.goal_cells[p.park_index[b]]) {
        a = te;
        while (a > t0 && path[a - 1] == end) a--;
      }
      status[b] = f; arrive[b] = a; served[b] = done;
      fails += f > 0; late += a > T; sum += a; uns += n - done;
    }
    __syncthreads();
    timed_stamp(res, path, H, W, Wd, L, T, lag, rad, sep2, tid, nt);
    __syncthreads();
  }
  if (tid == 0) {
    p.key[g] = (int64_t)((fails << 44) | (late << 32) | sum);
    p.unserved[g] = (int)uns;
  }
}

// the order with the least (unserved, key, g) among the valid ones (a valid key is below INT64_MAX), -1 when there is none
__global__ __launch_bounds__(256) void k_timed_tours_best(const int64_t *__restrict__ key, const int *__restrict__ unserved,
                                                          int G, int *__restrict__ best) {
  __shared__ long long rk[256];
  __shared__ int ru[256], rg[256];
  const int tid = threadIdx.x;
  long long bk = INT64_MAX;
  int bu = INT_MAX, bg = -1;
  for (int g = tid; g < G; g += 256) {
    const long long k = key[g];
    const int u = unserved[g];
    if (k < INT64_MAX && (bg < 0 || u < bu || (u == bu && k < bk))) { bu = u; bk = k; bg = g; }     // (g ascends)
  }
  rk[tid] = bk; ru[tid] = bu; rg[tid] = bg;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      const long long k = rk[tid + h];
      const int u = ru[tid + h], g2 = rg[tid + h];
      if (g2 >= 0 && (rg[tid] < 0 || u < ru[tid] || (u == ru[tid] && (k < rk[tid] || (k == rk[tid] && g2 < rg[tid]))))) {
        rk[tid] = k; ru[tid] = u; rg[tid] = g2;
      }
    }
    __syncthreads();
  }
  if (tid == 0) *best = rg[0];
}

// k_timed_follow with the serve step: one workgroup per robot
__global__ __launch_bounds__(256) void k_timed_tours_follow(const int *__restrict__ paths, int B, int T, const int *__restrict__ idx_in,
                                                            int *__restrict__ idx_out, const double *__restrict__ pos, int stride,
                                                            int W, double x0, double y0, double cell, double threshold, int sep2,
                                                            int lag, double *__restrict__ goal, int *__restrict__ blocked, int K,
                                                            const int *__restrict__ serve_at, int *__restrict__ leg_io,
                                                            int *__restrict__ served, int now, double stop_tol) {
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
  const double dist = sqrt(dx * dx + dy * dy);
  const int *const sa = serve_at + (size_t)b * K;
  // the serve step (every thread decides the same; thread 0 writes)
  int leg = leg_io[b];
  leg = leg < 0 ? 0 : leg;
  bool serve = false;
  if (leg < K && sa[leg] == i && dist <= stop_tol) { serve = true; leg++; }
  const bool pending = leg < K && sa[leg] == i;
  bool at_stop = false;
  for (int k = 0; k < K; k++) at_stop = at_stop || sa[k] == i;
  int blk = INT_MAX;
  bool advance = false;
  if (i < T && !pending && dist <= (at_stop ? stop_tol : threshold)) {       // (uniform over the workgroup)
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
    if (serve) { served[(size_t)b * K + leg - 1] = now; leg_io[b] = leg; }
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
