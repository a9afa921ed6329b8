// rmpc_timed_replan.hpp -- lifelong timed tours (include/rmpc_timed_replan.h), included by rmpc_world.hip
// behind rmpc_timed.hpp and rmpc_timed_tours.hpp: the reservation table as a public input (k_timed_reserve stamps given
// paths into it), and k_timed_tours_replan, which is k_timed_tours_plan on a table that starts filled, with kept
// robots, a begin layer per robot and the standing rule.  The layer sweep, end-cell reduction, backtrack and stamping
// are those of rmpc_timed.hpp, called as they stand.
//
// The standing rule asks of a cell c and a layer t whether c conflicts with the start of another active robot r with
// t <= begin[r] + lag.  until(c) = the largest begin[r] + lag over the robots whose start conflicts with c answers it for
// every robot but the one that owns the maximum; that one needs the second largest.  k_timed_standing writes this
// top-two per cell once per call (it does not depend on the order), and every order's workgroup builds the mask
// {c : until_b(c) >= t} from it: once per robot while every begin is 0, again only when t passes a value of until_b.

#include <climits>
#include <cstdint>

namespace rmpc {

constexpr int kTimedKept = -2, kTimedSkipped = -1;      // eff[b] of a robot that is not planned; else begin[b] + lag

// the part of the workspace behind the G orders' parts, written by k_timed_standing: eff[b] per robot, the top-two of
// eff over the robots, and the top-two per cell (value, owner, second value)
struct TimedStanding {
  int *eff;                  // [RMPC_TIMED_MAX_ROBOTS]
  int *all;                  // [4]: the largest eff, its owner, the second largest
  int *top;                  // [H W][3]
};

static inline long long timed_standing_words(int H, int W) {
  return (RMPC_TIMED_MAX_ROBOTS + 4 + 3 * (long long)H * W + 1) / 2;
}

__device__ __forceinline__ TimedStanding timed_standing_at(timed_word *base) {
  TimedStanding s;
  s.eff = (int *)base;
  s.all = s.eff + RMPC_TIMED_MAX_ROBOTS;
  s.top = s.all + 4;
  return s;
}

// until_b(c): the largest begin[r] + lag over the other planned robots whose start conflicts with c, -1 without one
__device__ __forceinline__ int timed_until(const int *__restrict__ top, int c, int b) {
  return top[3 * c + 1] == b ? top[3 * c + 2] : top[3 * c];
}

// One thread per cell; every workgroup first works out eff[] for all robots in LDS (the robots are few and the rule is a
// handful of loads), workgroup 0 also writes eff, its top-two and clash.
__global__ __launch_bounds__(256) void k_timed_standing(rmpc_timed_tours p, rmpc_timed_replan x, int Wd, int L,
                                                        timed_word *__restrict__ shared) {
  __shared__ int eff[RMPC_TIMED_MAX_ROBOTS];
  const int tid = threadIdx.x, H = p.H, W = p.W, HW = H * W, B = p.B, T = p.T;
  const TimedStanding st = timed_standing_at(shared);
  for (int b = tid; b < B; b += 256) {
    const int bg = x.begin ? x.begin[b] : 0;
    int e = bg + p.lag;
    if (x.active && x.active[b] == 0) e = kTimedKept;
    else if (bg < 0 || bg > T || timed_tours_skipped(p, b, HW)) e = kTimedSkipped;
    eff[b] = e;
    if (blockIdx.x == 0) {
      st.eff[b] = e;
      if (x.clash) {
        int cl = 0;
        if (e >= 0 && x.res0) {
          const int s = p.start_cell[b], r = s / W, col = s - r * W;
          cl = (int)((x.res0[(size_t)bg * L + r * Wd + (col >> 6)] >> (col & 63)) & 1ull);
        }
        x.clash[b] = cl;
      }
    }
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0) {
    int v1 = -1, o1 = -1, v2 = -1;
    for (int b = 0; b < B; b++) {
      const int e = eff[b];
      if (e > v1) { v2 = v1; v1 = e; o1 = b; }
      else if (e > v2) v2 = e;
    }
    st.all[0] = v1; st.all[1] = o1; st.all[2] = v2;
  }
  const int c = blockIdx.x * 256 + tid;
  if (c >= HW) return;
  const int r0 = c / W, c0 = c - r0 * W;
  int v1 = -1, o1 = -1, v2 = -1;
  for (int b = 0; b < B; b++) {
    const int e = eff[b];
    if (e < 0) continue;
    const int s = p.start_cell[b], dr = s / W - r0, dc = s % W - c0;
    if (dr * dr + dc * dc >= p.sep2) continue;       // (|dr|, |dc| < 16384: no overflow)
    if (e > v1) { v2 = v1; v1 = e; o1 = b; }
    else if (e > v2) v2 = e;
  }
  st.top[3 * c] = v1; st.top[3 * c + 1] = o1; st.top[3 * c + 2] = v2;
}

// mask[w] = the cells with until_b(c) >= t; returns this thread's least until_b(c) >= t (INT_MAX without one): the mask
// holds for every layer up to the least of them
__device__ __forceinline__ int timed_standing_mask(const int *__restrict__ top, int b, int t, timed_word *__restrict__ mask,
                                                   int W, int Wd, int L, int tid, int nt) {
  int least = INT_MAX;
  for (int w = tid; w < L; w += nt) {
    const int r = w / Wd, c0 = (w - r * Wd) * 64;
    timed_word word = 0;
    for (int bb = 0; bb < 64 && c0 + bb < W; bb++) {
      const int u = timed_until(top, r * W + c0 + bb, b);
      if (u >= t) { word |= 1ull << bb; least = u < least ? u : least; }
    }
    mask[w] = word;
  }
  return least;
}

// One workgroup per path: rule 8 for the cells that lie on the map
__global__ __launch_bounds__(kTimedThreads) void k_timed_reserve(int H, int W, int T, const int *__restrict__ cells,
                                                                 const int *__restrict__ use, int sep2, int lag, int rad,
                                                                 int Wd, int L, timed_word *__restrict__ res) {
  const int p = blockIdx.x;
  if (use && use[p] == 0) return;
  timed_stamp<true>(res, cells + (size_t)p * (T + 1), H, W, Wd, L, T, lag, rad, sep2, threadIdx.x, kTimedThreads);
}

// One workgroup per priority order, as k_timed_tours_plan; `mask` is the workspace's word row that holds `later` there.
template <bool kLds>
__global__ __launch_bounds__(kTimedThreads) void k_timed_tours_replan(rmpc_timed_tours p, rmpc_timed_replan x, TimedGeom q,
                                                                      timed_word *__restrict__ work) {
#pragma clang fp contract(off)
  extern __shared__ timed_word timed_lds[];
  __shared__ unsigned seen[RMPC_TIMED_MAX_ROBOTS / 32];
  __shared__ double red_d[kTimedThreads];
  __shared__ int red_c[kTimedThreads];
  __shared__ int mask_least;
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
  timed_word *const mask = freeb + L;
  const TimedStanding st = timed_standing_at(work + (size_t)gridDim.x * q.per_order);

  for (size_t i = tid; i < (size_t)(T + 1) * L; i += nt) res[i] = x.res0 ? x.res0[i] : 0ull;
  for (int w = tid; w < L; w += nt) {
    const int r = w / Wd, c0 = (w - r * Wd) * 64;
    timed_word word = 0;
    for (int b = 0; b < 64 && c0 + b < W; b++)
      if (!(p.grid[r * W + c0 + b] >= p.occ_threshold)) word |= 1ull << b;
    freeb[w] = word;
  }
  __syncthreads();

  long long fails = 0, late = 0, sum = 0, uns = 0;       // (thread 0's)
  for (int k = 0; k < B; k++) {
    const int b = ord[k], n = p.len[b], e = st.eff[b];
    int *const path = paths + (size_t)b * (T + 1);
    int *const sa = serve_at + (size_t)b * K;
    for (int j = tid; j < K; j += nt) sa[j] = -1;
    if (e < 0) {
      for (int t = tid; t <= T; t += nt) path[t] = -1;
      if (tid == 0) {
        served[b] = 0;
        if (e == kTimedKept) { status[b] = RMPC_TIMED_KEPT; arrive[b] = 0; }
        else {
          status[b] = RMPC_GRID_OUTSIDE; arrive[b] = T + 1;
          late++; sum += T + 1; uns += n >= 0 && n <= K ? n : 0;
        }
      }
      continue;
    }
    const int s = p.start_cell[b], begin = e - lag;
    // the standing rule binds up to the largest begin + lag of the other planned robots
    const int bound = st.all[1] == b ? st.all[2] : st.all[0];
    int mask_to = -1;                  // the mask in `mask` holds for the layers up to this one
    for (int t = tid; t < begin; t += nt) path[t] = s;

    int t0 = begin, at = s, done = 0;  // the state; done: stops served
    int f = 0, te = 0, end = 0;        // how the last leg ended
    bool failed = false;
    for (int j = 0; j <= n && !failed; j++) {              // leg n is the parking leg (rule 4)
      const bool parking = j == n;
      const int gi = parking ? p.park_index[b] : p.stops[(size_t)b * K + j];
      const int sc = parking ? -1 : p.goal_cells[gi];
      const bool inside = sc >= 0 && sc < HW;              // a stop outside the map is in no layer
      const int sw = inside ? (sc / W) * Wd + ((sc % W) >> 6) : 0;
      const timed_word sbit = inside ? 1ull << ((sc % W) & 63) : 0ull;
      timed_seed_layer(hist + (size_t)t0 * L, Wd, L, at / W, at % W, tid, nt);
      __syncthreads();
      int a = -1;
      f = 0;
      for (int t = t0; t <= T; t++) {                      // at most T - t0 layers
        if (t > t0) {
          const bool early = t <= bound;
          if (early && t > mask_to) {                      // (uniform)
            if (tid == 0) mask_least = INT_MAX;
            __syncthreads();
            const int least = timed_standing_mask(st.top, b, t, mask, W, Wd, L, tid, nt);
            if (least != INT_MAX) atomicMin(&mask_least, least);
            __syncthreads();
            mask_to = mask_least == INT_MAX ? bound : mask_least;
          }
          const bool any = timed_sweep_layer(hist + (size_t)(t - 1) * L, hist + (size_t)t * L, res + (size_t)t * L, freeb,
                                             mask, early, H, Wd, L, p.movement, tid, nt);
          if (!__syncthreads_or(any)) { f = t; break; }
        }
        if (!parking && t + dwell <= T && (hist[(size_t)t * L + sw] & sbit)) {
          bool held = true;
          const int until = timed_until(st.top, sc, b);
          for (int u = t + 1; u <= t + dwell && held; u++) {
            if (__hip_atomic_load(res + (size_t)u * L + sw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & sbit) held = false;
            if (u <= until) held = false;
          }
          if (held) { a = t; break; }
        }
      }
      if (a < 0) {
        // rules 3 and 4: the robot goes as near the leg's goal as it got and stays
        te = f ? f - 1 : T;
        end = timed_end_cell(p.fields + (size_t)gi * HW, hist + (size_t)te * L, W, Wd, L, red_d, red_c, tid, nt);
        failed = !parking;
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

}  // namespace rmpc
