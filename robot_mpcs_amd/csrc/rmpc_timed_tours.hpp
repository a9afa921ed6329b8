// rmpc_timed_tours.hpp -- timed tours (include/rmpc_timed_tours.h), included by rmpc_world.hip behind
// rmpc_timed.hpp: the plan of rmpc_timed.hpp with a sequence of stops per robot, and the follower with the serve step.
// The route of a robot through its stops is timed_robot of rmpc_timed.hpp under the later-starts rule, which k_timed_plan
// calls without stops; what is here is where the tours' inputs and outputs live (rule 1, the outputs of an order, the
// serve-time rows) and the serve step.  What a stop adds to a layer is uniform over the workgroup: one bit test of the
// stop's cell, and up to `dwell` loads of res.

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

// the outputs of order g
__device__ __forceinline__ TimedOut timed_tours_out(const rmpc_timed_tours &p, int g) {
  const size_t gB = (size_t)g * p.B;
  return {p.status + gB, p.arrive + gB, p.paths + gB * (p.T + 1), p.key + g, p.served + gB, p.serve_at + gB * p.K, p.unserved + g};
}

// robot b of an order under `rule`, prepared for it: its route from start_cell[b] at layer begin, its outputs and its
// part of the key
template <class Rule>
__device__ __forceinline__ void timed_tours_robot(const rmpc_timed_tours &p, const TimedOut &o, const TimedDims &d,
                                                  const TimedWork &wk, Rule &rule, int b, int begin, TimedKey &key,
                                                  double *red_d, int *red_c) {
  const int n = p.len[b];
  const TimedEnd e = timed_robot<true>(d, wk, rule, p.fields, p.goal_cells, p.start_cell[b], begin, n, p.stops + (size_t)b * p.K,
                                       p.park_index[b], p.dwell, o.paths + (size_t)b * (d.T + 1), o.serve_at + (size_t)b * p.K,
                                       o.status + b, o.arrive + b, red_d, red_c);
  if (d.tid == 0) { o.served[b] = e.done; key.planned(e.f, e.a, d.T, n, e.done); }
}

// One workgroup per priority order, as k_timed_plan.  The history holds the layers of the current leg only: a leg writes
// the layers from its t0 on, and its backtrack is taken before the next leg begins.
template <bool kLds>
__global__ __launch_bounds__(kTimedThreads) void k_timed_tours_plan(rmpc_timed_tours p, TimedGeom q, timed_word *__restrict__ work) {
  __shared__ double red_d[kTimedThreads];
  __shared__ int red_c[kTimedThreads];
  const int g = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, B = p.B, T = p.T, K = p.K, HW = p.H * p.W;
  const TimedDims d = {p.H, p.W, q.Wd, q.L, T, p.lag, p.sep2, q.rad, p.movement, tid, nt};
  const int *const ord = p.orders + (size_t)g * B;
  const TimedOut o = timed_tours_out(p, g);
  if (timed_order_bad(ord, B, tid, nt)) {
    timed_bad_order<true>(o, B, T, K, tid, nt);
    return;
  }

  const TimedWork wk = timed_work_at<kLds>(work, g, q, T);
  for (size_t i = tid; i < (size_t)(T + 1) * d.L; i += nt) wk.res[i] = 0;
  timed_free_mask(wk.freeb, p.grid, p.occ_threshold, d);
  TimedLaterStarts rule = {d, wk.cnt, wk.mask};
  rule.count(ord, p.start_cell, B, [&](int b) { return timed_tours_skipped(p, b, HW); });

  TimedKey key;
  for (int k = 0; k < B; k++) {
    const int b = ord[k];
    for (int j = tid; j < K; j += nt) o.serve_at[(size_t)b * K + j] = -1;
    if (timed_tours_skipped(p, b, HW)) {
      for (int t = tid; t <= T; t += nt) o.paths[(size_t)b * (T + 1) + t] = -1;
      if (tid == 0) {
        o.status[b] = RMPC_GRID_OUTSIDE; o.arrive[b] = T + 1; o.served[b] = 0;
        key.skipped(T, p.len[b], K);
      }
      continue;
    }
    rule.prepare(b, p.start_cell[b]);
    timed_tours_robot(p, o, d, wk, rule, b, 0, key, red_d, red_c);
  }
  if (tid == 0) { *o.key = key.key(); *o.unserved = (int)key.uns; }
}

__global__ __launch_bounds__(256) void k_timed_tours_best(const int64_t *__restrict__ key, const int *__restrict__ unserved,
                                                          int G, int *__restrict__ best) {
  __shared__ long long rk[256];
  __shared__ int ru[256], rg[256];
  timed_best_order<true>(key, unserved, G, best, rk, ru, rg);
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
  const double dist = timed_waypoint_dist(p, T, i, pos + (size_t)b * stride, W, x0, y0, cell);
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
    blk = timed_blocker(paths, B, T, idx_in, b, p, i, W, sep2, lag, red);
    advance = blk == INT_MAX;
  }
  if (tid == 0) {
    if (serve) { served[(size_t)b * K + leg - 1] = now; leg_io[b] = leg; }
    timed_goal_write(p, advance ? i + 1 : i, blk, b, idx_out, goal, blocked, W, x0, y0, cell);
  }
}

}  // namespace rmpc
