// rmpc_track.hpp -- moving obstacles from a lidar scan, included by rmpc_world.hip: the moving returns of
// one scan, their segments, a circle of known radius per segment, an alpha-beta filter per track and the obst_dyn rows a
// scene points at.  The rules are include/rmpc.h's (rmpc_tracks) and the project's own; tests/tracking_reference.py
// restates them.  Contraction is off and the arithmetic is + - * / sqrt on doubles: the kernel evaluates the
// restatement's expressions in the restatement's order.

namespace rmpc {

constexpr int kTrackThreads = 256;
constexpr int kTrackMaxRays = RMPC_TRACK_MAX_RAYS, kTrackWords = RMPC_TRACK_MAX_RAYS / 64;
constexpr int kTrackMaxT = RMPC_TRACK_MAX_TRACKS, kTrackMaxDet = RMPC_TRACK_MAX_DET;
static_assert(kTrackMaxT * kTrackMaxDet == kTrackThreads, "one lane per (track, detection) pair");
static_assert(kTrackWords <= 64, "the word scans are done by the lanes of one wave");

// the least set bit of the words e[0 .. nw) at a position in [from, R), -1 when there is none (bits past R are clear)
__device__ __forceinline__ int track_next_bit(const unsigned long long *e, int nw, int from) {
  for (int w = from >> 6; w < nw; w++) {
    unsigned long long x = e[w];
    if (w == (from >> 6)) x &= ~0ull << (from & 63);
    if (x) return (w << 6) + __ffsll((long long)x) - 1;
  }
  return -1;
}

// the length of the segment that starts at ray i: to the next end (a start or a ray that is not moving), around the seam
// of a closed sweep, where ray i itself ends the search at the latest
__device__ __forceinline__ int track_seg_len(const unsigned long long *e, int nw, int R, bool closed, int i) {
  const int j = i + 1 < R ? track_next_bit(e, nw, i + 1) : -1;
  if (j >= 0) return j - i;
  return closed ? track_next_bit(e, nw, 0) + R - i : R - i;
}

// One workgroup per robot.  Lanes over rays: a wave's 64 rays are one 64-bit word of the moving, start and keep flags
// (__ballot), so that a segment's length is a bit scan over at most 32 words and its rank a popcount.  x and y of the
// points are staged in LDS (2 x 16 KB at 2048 rays): the start test, the extent test and the fits read them there.
// One lane per detection fits its circle sequentially in segment order -- the sums are the restatement's sums.  One
// lane per (track, detection) pair holds a squared distance; the sequential greedy rule takes the least (s, j, k) of
// the pairs whose sides are both untaken, which is what a round's block-wide minimum finds: at most 16 rounds.
__global__ __launch_bounds__(kTrackThreads) void k_lidar_tracks(rmpc_tracks a) {
#pragma clang fp contract(off)
  __shared__ double s_x[kTrackMaxRays], s_y[kTrackMaxRays];
  __shared__ unsigned long long s_mov[kTrackWords], s_st[kTrackWords], s_end[kTrackWords], s_keep[kTrackWords];
  __shared__ int s_pre[kTrackWords];                           // kept starts before the word
  __shared__ int s_nseg, s_nkept;
  __shared__ int s_seg0[kTrackMaxDet], s_segn[kTrackMaxDet];
  __shared__ double s_zx[kTrackMaxDet], s_zy[kTrackMaxDet];
  __shared__ double s_tr[kTrackMaxT][4], s_px[kTrackMaxT], s_py[kTrackMaxT], s_d2[kTrackMaxT];
  __shared__ int s_age[kTrackMaxT], s_miss[kTrackMaxT], s_mj[kTrackMaxT], s_mk[kTrackMaxDet];
  __shared__ unsigned long long s_rk[kTrackThreads / 64];
  __shared__ int s_ri[kTrackThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, R = a.rays, T = a.n_tracks;
  const int nw = (R + 63) >> 6, Rpad = nw << 6;
  const bool closed = a.closed != 0;
  const double *const pts = a.points + (size_t)b * R * 3;
  const double *const rng = a.ranges + (size_t)b * R;
  const double *const srng = a.static_ranges ? a.static_ranges + (size_t)b * R : nullptr;
  const double ox = a.origin[(size_t)b * 3], oy = a.origin[(size_t)b * 3 + 1];

  // the filter's state, and the marks of the association
  if (tid < T) {
    const size_t g = (size_t)b * T + tid;
    for (int c = 0; c < 4; c++) s_tr[tid][c] = a.track[g * 4 + c];
    s_age[tid] = a.age[g];
    s_miss[tid] = a.miss[g];
    s_mj[tid] = -1;
  }
  if (tid < kTrackMaxDet) s_mk[tid] = -1;

  // 1. moving rays (whole waves walk the padded sweep: a ballot is one word)
  for (int i = tid; i < Rpad; i += kTrackThreads) {
    bool mv = false;
    if (i < R) {
      const double t = rng[i];
      s_x[i] = pts[3 * i];
      s_y[i] = pts[3 * i + 1];
      mv = srng ? t < srng[i] - a.margin : t < a.range;
    }
    const unsigned long long w = __ballot(mv);
    if (lane == 0) s_mov[i >> 6] = w;
  }
  __syncthreads();

  // 2. starts
  const double gap2 = a.gap * a.gap;
  for (int i = tid; i < Rpad; i += kTrackThreads) {
    bool st = false;
    if (i < R && (s_mov[i >> 6] >> (i & 63) & 1)) {
      const int pr = i > 0 ? i - 1 : (closed ? R - 1 : -1);
      bool link = false;
      if (pr >= 0 && (s_mov[pr >> 6] >> (pr & 63) & 1)) {
        const double dx = s_x[i] - s_x[pr], dy = s_y[i] - s_y[pr];
        link = (dx * dx + dy * dy) <= gap2;
      }
      st = !link;
    }
    const unsigned long long w = __ballot(st);
    if (lane == 0) s_st[i >> 6] = w;
  }
  __syncthreads();
  if (tid < 64) {
    // the first wave: the ring without a start, the segment ends, and the number of starts
    const unsigned long long valid = tid < nw ? (tid == nw - 1 && (R & 63) ? ~0ull >> (64 - (R & 63)) : ~0ull) : 0ull;
    unsigned long long mv = tid < nw ? s_mov[tid] : 0ull, st = tid < nw ? s_st[tid] : 0ull;
    const bool ring = closed && __ballot(tid < nw && mv != valid) == 0ull && __ballot(st != 0ull) == 0ull;
    if (ring && tid == 0) { st = 1ull; s_st[0] = st; }
    if (tid < nw) s_end[tid] = (st | ~mv) & valid;
    int inc = __popcll(st);
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(inc, o);
      if (tid >= o) inc += v;
    }
    if (tid == 63) s_nseg = inc;
  }
  __syncthreads();

  // segment lengths and the drops; a kept start votes into s_keep
  const double me2 = a.max_extent * a.max_extent;
  for (int i = tid; i < Rpad; i += kTrackThreads) {
    bool keep = false;
    if (i < R && (s_st[i >> 6] >> (i & 63) & 1)) {
      const int n = track_seg_len(s_end, nw, R, closed, i);
      keep = n >= a.min_rays;
      if (keep && a.max_extent > 0.0) {
        int l = i + n - 1;
        l = l >= R ? l - R : l;
        const double dx = s_x[l] - s_x[i], dy = s_y[l] - s_y[i];
        keep = !((dx * dx + dy * dy) > me2);
      }
    }
    const unsigned long long w = __ballot(keep);
    if (lane == 0) s_keep[i >> 6] = w;
  }
  __syncthreads();
  if (tid < 64) {
    const unsigned long long kp = tid < nw ? s_keep[tid] : 0ull;
    int inc = __popcll(kp);
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(inc, o);
      if (tid >= o) inc += v;
    }
    if (tid < nw) s_pre[tid] = inc - __popcll(kp);
    if (tid == 63) s_nkept = inc;
  }
  __syncthreads();
  for (int i = tid; i < R; i += kTrackThreads) {
    const unsigned long long kp = s_keep[i >> 6];
    if (kp >> (i & 63) & 1) {
      const int rank = s_pre[i >> 6] + __popcll(kp & ((1ull << (i & 63)) - 1ull));
      if (rank < kTrackMaxDet) {
        s_seg0[rank] = i;
        s_segn[rank] = track_seg_len(s_end, nw, R, closed, i);
      }
    }
  }
  __syncthreads();
  const int ndet = min(s_nkept, kTrackMaxDet);

  // 3. one lane per detection: the circle of the known radius
  if (tid < ndet) {
    const int s0 = s_seg0[tid], n = s_segn[tid];
    double sx = 0.0, sy = 0.0;
    for (int t = 0, i = s0; t < n; t++) {
      sx = sx + s_x[i];
      sy = sy + s_y[i];
      i = i + 1 == R ? 0 : i + 1;
    }
    const double mx = sx / (double)n, my = sy / (double)n;
    const double wx = mx - ox, wy = my - oy;
    const double nrm = sqrt(wx * wx + wy * wy);
    double cx = mx + a.radius * (wx / nrm), cy = my + a.radius * (wy / nrm);
    for (int it = 0; it < 4; it++) {
      double a11 = 0.0, a12 = 0.0, a22 = 0.0, gx = 0.0, gy = 0.0;
      for (int t = 0, i = s0; t < n; t++) {
        const double qx = s_x[i] - cx, qy = s_y[i] - cy;
        const double r = sqrt(qx * qx + qy * qy);
        const double ux = qx / r, uy = qy / r;
        const double e = r - a.radius;
        a11 = a11 + ux * ux;
        a12 = a12 + ux * uy;
        a22 = a22 + uy * uy;
        gx = gx + ux * e;
        gy = gy + uy * e;
        i = i + 1 == R ? 0 : i + 1;
      }
      a11 = a11 + 1e-3;
      a22 = a22 + 1e-3;
      const double D = a11 * a22 - a12 * a12;
      cx = cx + (a22 * gx - a12 * gy) / D;
      cy = cy + (a11 * gy - a12 * gx) / D;
    }
    s_zx[tid] = cx;
    s_zy[tid] = cy;
  }
  // 4. predict
  if (tid < T) {
    s_px[tid] = s_tr[tid][0] + s_tr[tid][2] * a.dt;
    s_py[tid] = s_tr[tid][1] + s_tr[tid][3] * a.dt;
  }
  __syncthreads();

  // associate: lane (j, k); s >= +0 orders as its bits
  {
    const int j = tid >> 4, k = tid & 15;
    const unsigned long long none = ~0ull;
    unsigned long long key = none;
    if (j < T && k < ndet && s_age[j] > 0) {
      const double dx = s_px[j] - s_zx[k], dy = s_py[j] - s_zy[k];
      const double s = dx * dx + dy * dy;
      if (s <= a.gate * a.gate) key = (unsigned long long)__double_as_longlong(s);
    }
    for (int round = 0; round < kTrackMaxDet; round++) {
      unsigned long long bk = key;
      int bi = tid;
      for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ok = __shfl_xor(bk, off);
        const int oi = __shfl_xor(bi, off);
        if (ok < bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; }
      }
      if (lane == 0) { s_rk[tid >> 6] = bk; s_ri[tid >> 6] = bi; }
      __syncthreads();
      bk = s_rk[0]; bi = s_ri[0];
      for (int w = 1; w < kTrackThreads / 64; w++) {
        const unsigned long long ok = s_rk[w];
        const int oi = s_ri[w];
        if (ok < bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; }
      }
      __syncthreads();                                       // s_rk is written again in the next round
      if (bk == none) break;                                 // (uniform)
      const int wj = bi >> 4, wk = bi & 15;
      if (tid == bi) { s_mj[wj] = wk; s_mk[wk] = wj; }
      if (j == wj || k == wk) key = none;
    }
  }
  __syncthreads();

  // update or coast
  if (tid < T && s_age[tid] > 0) {
    const int k = s_mj[tid];
    if (k >= 0) {
      const double rx = s_zx[k] - s_px[tid], ry = s_zy[k] - s_py[tid];
      double vx = s_tr[tid][2] + (a.beta * rx) / a.dt, vy = s_tr[tid][3] + (a.beta * ry) / a.dt;
      if (a.v_max > 0.0) {
        if (vx > a.v_max) vx = a.v_max;
        if (vx < -a.v_max) vx = -a.v_max;
        if (vy > a.v_max) vy = a.v_max;
        if (vy < -a.v_max) vy = -a.v_max;
      }
      s_tr[tid][0] = s_px[tid] + a.alpha * rx;
      s_tr[tid][1] = s_py[tid] + a.alpha * ry;
      s_tr[tid][2] = vx;
      s_tr[tid][3] = vy;
      s_age[tid] = s_age[tid] == INT_MAX ? INT_MAX : s_age[tid] + 1;
      s_miss[tid] = 0;
    } else {
      s_tr[tid][0] = s_px[tid];
      s_tr[tid][1] = s_py[tid];
      const int ms = s_miss[tid] == INT_MAX ? INT_MAX : s_miss[tid] + 1;
      s_miss[tid] = ms;
      if (ms > a.max_miss) s_age[tid] = 0;
    }
  }
  __syncthreads();
  // births: sequential by definition (detection order into the lowest free slots), at most 16 x 16 steps
  if (tid == 0) {
    int j = 0;
    for (int k = 0; k < ndet; k++) {
      if (s_mk[k] >= 0) continue;
      while (j < T && s_age[j] != 0) j++;
      if (j >= T) break;
      s_tr[j][0] = s_zx[k]; s_tr[j][1] = s_zy[k]; s_tr[j][2] = 0.0; s_tr[j][3] = 0.0;
      s_age[j] = 1;
      s_miss[j] = 0;
    }
  }
  __syncthreads();

  // 5. the state back, and the confirmed tracks by distance from the sensor
  bool conf = false, alive = false;
  if (tid < T) {
    const size_t g = (size_t)b * T + tid;
    for (int c = 0; c < 4; c++) a.track[g * 4 + c] = s_tr[tid][c];
    a.age[g] = s_age[tid];
    a.miss[g] = s_miss[tid];
    alive = s_age[tid] > 0;
    conf = s_age[tid] >= a.confirm;
    const double dx = s_tr[tid][0] - ox, dy = s_tr[tid][1] - oy;
    const double s = dx * dx + dy * dy;
    s_d2[tid] = conf ? (s == s ? s : __builtin_inf()) : -1.0;      // -1: not confirmed
  }
  const int nlive = __syncthreads_count(alive);
  const int nconf = __syncthreads_count(conf);
  double *const od = a.obst_dyn + (size_t)b * a.n_out * 9;
  if (conf) {
    const double s = s_d2[tid];
    int rank = 0;
    for (int j = 0; j < T; j++) {
      const double sj = s_d2[j];
      rank += sj >= 0.0 && (sj < s || (sj == s && j < tid)) ? 1 : 0;
    }
    if (rank < a.n_out) {
      double *const o = od + (size_t)rank * 9;
      o[0] = s_tr[tid][0]; o[1] = s_tr[tid][1]; o[2] = 0.0;
      o[3] = s_tr[tid][2]; o[4] = s_tr[tid][3]; o[5] = 0.0;
      o[6] = 0.0; o[7] = 0.0; o[8] = 0.0;
    }
  }
  for (long long e = (long long)min(nconf, a.n_out) * 9 + tid; e < (long long)a.n_out * 9; e += kTrackThreads) {
    const int c = (int)(e % 9);
    od[e] = c == 0 ? a.park_x : (c == 1 ? a.park_y : 0.0);
  }
  if (a.det)
    for (int e = tid; e < kTrackMaxDet * 2; e += kTrackThreads) {
      const int k = e >> 1;
      a.det[(size_t)b * kTrackMaxDet * 2 + e] = k < ndet ? (e & 1 ? s_zy[k] : s_zx[k]) : 0.0;
    }
  if (a.counts && tid == 0) {
    int *const c = a.counts + (size_t)b * 4;
    c[0] = s_nseg; c[1] = ndet; c[2] = nlive; c[3] = nconf;
  }
}

}  // namespace rmpc
