// rmpc_locate.hpp -- localisation on the device, included by rmpc_world.hip behind rmpc_map.hpp: the
// likelihood field of an occupancy grid as exact integers (k_edge_distance), a scan's ranges re-projected at a believed
// pose (k_lidar_project, the expressions of k_lidar) and correlative scan matching over a lattice of poses around that
// pose (k_scan_match; Olson 2009, the brute-force half).  A score is an int32 sum of table entries and the choice a
// minimum of one 64-bit key, so no result depends on the order in which lanes meet.  Contraction is off in every
// function here: the kernels evaluate the restatement's expressions (tests/localization_reference.py).

namespace rmpc {

constexpr int kEdgeTile = 256;          // fine cells of a row per workgroup
constexpr int kEdgeMaxWin = 256;        // ceil(sqrt(cap)) at cap = 65535
constexpr int kEdgeFar = 1 << 15;       // "no cell of the other class in this column": its square exceeds every cap
constexpr int kMatchThreads = 256;
constexpr int kMatchMaxRays = RMPC_MATCH_MAX_RAYS;
constexpr int kMatchMaxN = 15;          // nxy, nth <= 15: k < 31^3 = 29 791 < 2^15 and m <= 3 * 225 = 675 < 2^10
static_assert(2 * kMatchMaxRays * sizeof(double) <= 48 * 1024, "k_scan_match: (ux, uy) of every ray staged in LDS");

// Fine cell (R, C) of the grid cut into sub x sub has the class data [R / sub][C / sub] >= occ_threshold (false for a
// NaN); d2 [R][C] = min(cap, least (R - R')^2 + (C - C')^2 over the fine cells of the other class inside the map).
// Separable: v(R, C') = the least |R - R'| to a cell of column C' whose class differs from that of (R, C') itself, then
// d2 (R, C) = min over C' of (C - C')^2 + (class(R, C') != class(R, C) ? 0 : v(R, C')^2).  Both searches stop at
// win = ceil(sqrt(cap)) fine cells: an offset beyond it has a square >= cap.  One workgroup per (row, tile of kEdgeTile
// columns): the vertical distances of the tile and of win columns on either side go through LDS; the coarse grid (at
// most 128 KiB) is read through the caches.
__global__ __launch_bounds__(256) void k_edge_distance(const double *__restrict__ grid, int H, int W, double occ_threshold,
                                                       int sub, int cap, int win, int ntile, int *__restrict__ d2) {
#pragma clang fp contract(off)
  __shared__ int s_v[kEdgeTile + 2 * kEdgeMaxWin];
  __shared__ signed char s_cls[kEdgeTile + 2 * kEdgeMaxWin];   // 0 free, 1 occupied, -1 outside the map
  const int tid = threadIdx.x;
  const int R = blockIdx.x / ntile, C0 = (blockIdx.x - R * ntile) * kEdgeTile;
  const int FH = H * sub, FW = W * sub;
  for (int i = tid; i < kEdgeTile + 2 * win; i += 256) {
    const int C = C0 - win + i;
    int v = kEdgeFar, cls = -1;
    if (C >= 0 && C < FW) {
      const int col = C / sub;
      cls = grid[(R / sub) * W + col] >= occ_threshold ? 1 : 0;
      for (int d = 1; d <= win; d++) {
        const bool up = R - d >= 0 && (grid[((R - d) / sub) * W + col] >= occ_threshold ? 1 : 0) != cls;
        const bool dn = R + d < FH && (grid[((R + d) / sub) * W + col] >= occ_threshold ? 1 : 0) != cls;
        if (up || dn) { v = d; break; }
      }
    }
    s_v[i] = v;
    s_cls[i] = (signed char)cls;
  }
  __syncthreads();
  const int C = C0 + tid;
  if (C >= FW) return;
  const int me = s_cls[win + tid];
  int best = cap;
  for (int j = -win; j <= win; j++) {
    const int c = s_cls[win + tid + j];
    if (c < 0) continue;
    const int v = c == me ? s_v[win + tid + j] : 0;
    const int d = j * j + v * v;                    // <= 2^16 + 2^30
    best = d < best ? d : best;
  }
  d2[R * FW + C] = best;
}

// One lane per (robot, ray): the point of the range t = ranges [b][i] along ray i of the pose, in k_lidar's expressions
// (the same origin, angle and direction, so the scan's pose and ranges give the scan's points bit for bit).
__global__ __launch_bounds__(256) void k_lidar_project(const double *__restrict__ pose, int stride, int B, int R,
                                                       double amin, double step, double offx, double offy, double height,
                                                       const double *__restrict__ ranges, double *__restrict__ points) {
#pragma clang fp contract(off)
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= B * R) return;
  const int b = g / R, i = g - b * R;
  const double *const p = pose + (size_t)b * stride;
  const double x = p[0], y = p[1], th = p[2];
  double ox, oy;
  sense_origin(x, y, cos(th), sin(th), offx, offy, ox, oy);
  const double ang = (th + amin) + (double)i * step;
  const double dx = cos(ang), dy = sin(ang);
  const double t = ranges[g];
  double *const o = points + (size_t)g * 3;
  o[0] = ox + t * dx;
  o[1] = oy + t * dy;
  o[2] = height;
}

// the fine cell coordinate of a world coordinate, as a double: compared against the map before it becomes an int
__device__ __forceinline__ double match_fine(double q, double q0, double cell, double sub) {
#pragma clang fp contract(off)
  return floor(((q - q0) / cell + 0.5) * sub);
}

// One workgroup per robot (include/rmpc.h, rmpc_scan_match).  The robot's used rays, as (ux, uy) relative to the prior
// position, are compacted into LDS once (in any order: a score is an integer sum).  Candidate k goes to thread k % 256,
// jx fastest: the lanes of a wave walk the rays together, so an LDS read is one broadcast word and the gathered fine
// cells of a ray are neighbours in d2, which stays in global memory (the table is shared by the whole fleet).  The least
// (score, m, k) is the minimum of the key score << 25 | m << 15 | k: within a thread, then by shuffles in the wave, then
// over the four waves through LDS.
__global__ __launch_bounds__(kMatchThreads) void k_scan_match(rmpc_scan_match m) {
#pragma clang fp contract(off)
  __shared__ double s_ux[kMatchMaxRays], s_uy[kMatchMaxRays];
  __shared__ unsigned long long s_key[kMatchThreads / 64];
  __shared__ int s_n;
  const int b = blockIdx.x, tid = threadIdx.x, R = m.rays;
  const double *const p = m.pose + (size_t)b * m.pose_stride;
  const double x = p[0], y = p[1], th = p[2];
  if (tid == 0) s_n = 0;
  __syncthreads();
  for (int i = tid; i < R; i += kMatchThreads) {
    const size_t g = (size_t)b * R + i;
    const double t = m.ranges[g], px = m.points[3 * g], py = m.points[3 * g + 1];
    if (isfinite(t) && isfinite(px) && isfinite(py) && t > 0.0 && t < m.range) {
      const int slot = atomicAdd(&s_n, 1);
      s_ux[slot] = px - x;
      s_uy[slot] = py - y;
    }
  }
  __syncthreads();
  const int n = s_n;
  if (n < m.min_hits) {                              // (the whole workgroup: n is uniform)
    if (tid == 0) {
      double *const o = m.pose_out + (size_t)b * 3;
      o[0] = x; o[1] = y; o[2] = th;
      m.best[b] = -1;
      m.score[b] = 0;
      if (m.score0) m.score0[b] = 0;
      if (m.used) m.used[b] = n;
    }
    return;
  }
  const int nx = 2 * m.nxy + 1, K = (2 * m.nth + 1) * nx * nx;
  const int k0 = (m.nth * nx + m.nxy) * nx + m.nxy;
  const int FW = m.W * m.sub;
  const double fw = (double)FW, fh = (double)(m.H * m.sub), sub = (double)m.sub;
  unsigned long long best = ~0ull;
  for (int k = tid; k < K; k += kMatchThreads) {
    const int jx = k % nx, jy = (k / nx) % nx, jth = k / (nx * nx);
    const int ix = jx - m.nxy, iy = jy - m.nxy, ith = jth - m.nth;
    const double c = m.rot[2 * jth], s = m.rot[2 * jth + 1];
    const double tx = x + (double)ix * m.step_xy, ty = y + (double)iy * m.step_xy;
    int score = 0;
    for (int j = 0; j < n; j++) {
      const double ux = s_ux[j], uy = s_uy[j];
      const double qx = (c * ux - s * uy) + tx;
      const double qy = (s * ux + c * uy) + ty;
      const double ca = match_fine(qx, m.x0, m.cell, sub), ra = match_fine(qy, m.y0, m.cell, sub);
      int v = m.cap;
      if (ca >= 0.0 && ca < fw && ra >= 0.0 && ra < fh) v = m.d2[(int)ra * FW + (int)ca];
      score += v;
    }
    if (k == k0 && m.score0) m.score0[b] = score;
    const unsigned long long key = (unsigned long long)score << 25 | (unsigned long long)(ix * ix + iy * iy + ith * ith) << 15 |
                                   (unsigned long long)k;
    best = key < best ? key : best;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_xor(best, off);
    best = other < best ? other : best;
  }
  if ((tid & 63) == 0) s_key[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kMatchThreads / 64; w++) best = s_key[w] < best ? s_key[w] : best;
    const int k = (int)(best & 0x7fffull);
    const int jx = k % nx, jy = (k / nx) % nx, jth = k / (nx * nx);
    double *const o = m.pose_out + (size_t)b * 3;
    o[0] = x + (double)(jx - m.nxy) * m.step_xy;
    o[1] = y + (double)(jy - m.nxy) * m.step_xy;
    o[2] = th + (double)(jth - m.nth) * m.step_th;
    m.best[b] = k;
    m.score[b] = (int)(best >> 25);
    if (m.used) m.used[b] = n;
  }
}

}  // namespace rmpc
