// rmpc_timed_replan.hpp -- lifelong timed tours (include/rmpc_timed_replan.h), included by rmpc_world.hip
// behind rmpc_timed.hpp and rmpc_timed_tours.hpp: the reservation table as a public input (k_timed_reserve stamps given
// paths into it), and k_timed_tours_replan, which is k_timed_tours_plan on a table that starts filled, with kept
// robots, a begin layer per robot and the standing rule.  The route of a robot is timed_robot of rmpc_timed.hpp, reached
// through timed_tours_robot of rmpc_timed_tours.hpp as in k_timed_tours_plan; the standing rule is its template
// parameter, TimedStandingRule below.
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

// The standing rule as a start rule of timed_robot (rmpc_timed.hpp): `mask` = the cells with until_b(c) >= t, rebuilt when
// t passes the least until_b(c) that it holds; it binds up to the largest begin + lag of the other planned robots.
struct TimedStandingRule {
  TimedDims d;
  TimedStanding st;
  timed_word *mask;
  int *mask_least;           // (one word of LDS) the least until_b(c) >= t over the cells of the mask
  int b, bound, mask_to;     // the robot, the last layer the rule binds in, the last layer the mask holds for

  __device__ __forceinline__ void prepare(int robot, int) {
    b = robot;
    bound = st.all[1] == b ? st.all[2] : st.all[0];
    mask_to = -1;
  }
  __device__ __forceinline__ bool early(int t) {
    const bool binds = t <= bound;
    if (binds && t > mask_to) {                          // (uniform)
      if (d.tid == 0) *mask_least = INT_MAX;
      __syncthreads();
      int least = INT_MAX;                               // this thread's
      const int *const top = st.top;
      const int robot = b;
      timed_pack_rows(mask, d, [&](int c) {
        const int u = timed_until(top, c, robot);
        if (u < t) return false;
        least = u < least ? u : least;
        return true;
      });
      if (least != INT_MAX) atomicMin(mask_least, least);
      __syncthreads();
      mask_to = *mask_least == INT_MAX ? bound : *mask_least;
    }
    return binds;
  }
  __device__ __forceinline__ int closed_until(int sc, int, timed_word) const { return timed_until(st.top, sc, b); }
};

// One workgroup per path: rule 8 for the cells that lie on the map
__global__ __launch_bounds__(kTimedThreads) void k_timed_reserve(int H, int W, int T, const int *__restrict__ cells,
                                                                 const int *__restrict__ use, int sep2, int lag, int rad,
                                                                 int Wd, int L, timed_word *__restrict__ res) {
  const int p = blockIdx.x;
  if (use && use[p] == 0) return;
  timed_stamp<true>(res, cells + (size_t)p * (T + 1), H, W, Wd, L, T, lag, rad, sep2, threadIdx.x, kTimedThreads);
}

// One workgroup per priority order, as k_timed_tours_plan, on a table that starts as res0, with kept robots, a begin
// layer per robot and the standing rule, whose mask is the workspace's word row that holds `later` there.
template <bool kLds>
__global__ __launch_bounds__(kTimedThreads) void k_timed_tours_replan(rmpc_timed_tours p, rmpc_timed_replan x, TimedGeom q,
                                                                      timed_word *__restrict__ work) {
  __shared__ double red_d[kTimedThreads];
  __shared__ int red_c[kTimedThreads];
  __shared__ int mask_least;
  const int g = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, B = p.B, T = p.T, K = p.K;
  const TimedDims d = {p.H, p.W, q.Wd, q.L, T, p.lag, p.sep2, q.rad, p.movement, tid, nt};
  const int *const ord = p.orders + (size_t)g * B;
  const TimedOut o = timed_tours_out(p, g);
  if (timed_order_bad(ord, B, tid, nt)) {
    timed_bad_order<true>(o, B, T, K, tid, nt);
    return;
  }

  const TimedWork wk = timed_work_at<kLds>(work, g, q, T);
  for (size_t i = tid; i < (size_t)(T + 1) * d.L; i += nt) wk.res[i] = x.res0 ? x.res0[i] : 0ull;
  timed_free_mask(wk.freeb, p.grid, p.occ_threshold, d);
  __syncthreads();
  TimedStandingRule rule = {d, timed_standing_at(work + (size_t)gridDim.x * q.per_order), wk.mask, &mask_least, 0, 0, 0};

  TimedKey key;
  for (int k = 0; k < B; k++) {
    const int b = ord[k], e = rule.st.eff[b];
    for (int j = tid; j < K; j += nt) o.serve_at[(size_t)b * K + j] = -1;
    if (e < 0) {
      for (int t = tid; t <= T; t += nt) o.paths[(size_t)b * (T + 1) + t] = -1;
      if (tid == 0) {
        o.served[b] = 0;
        if (e == kTimedKept) { o.status[b] = RMPC_TIMED_KEPT; o.arrive[b] = 0; }
        else {
          o.status[b] = RMPC_GRID_OUTSIDE; o.arrive[b] = T + 1;
          key.skipped(T, p.len[b], K);
        }
      }
      continue;
    }
    rule.prepare(b, p.start_cell[b]);
    timed_tours_robot(p, o, d, wk, rule, b, e - d.lag, key, red_d, red_c);
  }
  if (tid == 0) { *o.key = key.key(); *o.unserved = (int)key.uns; }
}

}  // namespace rmpc
