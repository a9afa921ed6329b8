// rmpc_any_angle.hpp -- line of sight on the grid and its two users (include/rmpc_any_angle.h), included
// by rmpc_world.hip: k_grid_visible answers pairs of cells, k_grid_shorten pulls a dense 8-connected route tight,
// k_follow_visible hands every robot the farthest route cell it can see.  The rule is the header's; the cell walk
// stands here once, templated on how a cell's occupancy is read.  Everything but the follower's distance test is
// integer arithmetic; contraction is off where doubles are formed, so all three are bitwise a plain restatement.
// Every loop is bounded (a walk by dx + dy <= H + W steps, the greedy loop by the path's length), no workgroup waits
// for another and there are no atomics.

namespace rmpc {

constexpr int kShortenLdsCells = 4096;     // a path of up to this many cells is read through LDS (16 KiB a wavefront)
constexpr int kFollowWaves = 4;            // robots per workgroup of k_follow_visible, a wavefront each

// occupancy from the doubles: the planner's test (a NaN is occupied)
struct OccGrid {
  const double *__restrict__ grid;
  int W;
  double occ_threshold;
  __device__ __forceinline__ bool operator()(int r, int c) const { return !(grid[r * W + c] < occ_threshold); }
};
// occupancy from the bit rows k_grid_occ_bits packs: word (r, c / 32), bit c % 32
struct OccBits {
  const unsigned *__restrict__ bits;
  int words;                               // words per row
  __device__ __forceinline__ bool operator()(int r, int c) const { return (bits[r * words + (c >> 5)] >> (c & 31)) & 1u; }
};

// visible((r0, c0), (r1, c1)) by the header's walk: every cell whose closed square the closed segment between the two
// centres meets, the first one apart; false at the first occupied one.  Both cells lie inside the map, and so does
// every cell the walk reads (they lie in the bounding box of the two).
template <class Occ>
__device__ __forceinline__ bool grid_visible(const Occ &occ, int r0, int c0, int r1, int c1) {
  int dx = c1 - c0, dy = r1 - r0;
  const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
  dx = dx < 0 ? -dx : dx;
  dy = dy < 0 ? -dy : dy;
  int e = dx - dy, n = dx + dy, r = r0, c = c0;
  dx *= 2;
  dy *= 2;
  while (n > 0) {
    if (e > 0) {
      c += sx; e -= dy; n -= 1;
    } else if (e < 0) {
      r += sy; e += dx; n -= 1;
    } else {                               // through a lattice corner: both side cells are touched
      if (occ(r, c + sx) || occ(r + sy, c)) return false;
      c += sx; r += sy; e += dx - dy; n -= 2;
    }
    if (occ(r, c)) return false;
  }
  return true;
}

__global__ __launch_bounds__(256) void k_grid_visible(const double *__restrict__ grid, int H, int W, double occ_threshold, int P,
                                                      const int *__restrict__ from, const int *__restrict__ to,
                                                      int *__restrict__ visible) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= P) return;
  const int HW = H * W, a = from[t], b = to[t];
  if (a < 0 || a >= HW || b < 0 || b >= HW) { visible[t] = -1; return; }
  visible[t] = grid_visible(OccGrid{grid, W, occ_threshold}, a / W, a % W, b / W, b % W) ? 1 : 0;
}

// the shortener's prologue: one wavefront per 64 cells of a row, a ballot is the two words
__global__ __launch_bounds__(256) void k_grid_occ_bits(const double *__restrict__ grid, int H, int W, double occ_threshold,
                                                       unsigned *__restrict__ bits) {
  const int lane = threadIdx.x & 63, words = (W + 31) >> 5, chunks = (W + 63) >> 6;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), r = wave / chunks, chunk = wave - r * chunks, c = chunk * 64 + lane;
  if (r >= H) return;                      // (the whole wavefront)
  const bool o = c < W && !(grid[(size_t)r * W + c] < occ_threshold);
  const unsigned long long m = __ballot(o);
  if (lane == 0) bits[r * words + 2 * chunk] = (unsigned)m;
  if (lane == 32 && 2 * chunk + 1 < words) bits[r * words + 2 * chunk + 1] = (unsigned)(m >> 32);
}

// One wavefront per path.  The path is checked first, whole (its length, every cell inside the map), and copied into
// LDS when kLds; an error row writes its code and no cell.  Then the header's greedy loop: the 64 lanes test the 64
// farthest candidates of the window (i + 1, hi] at once, lane l the index base + l, and the highest set bit of the
// ballot is the farthest visible one; the next chunk down is tested only when the ballot is empty, and when every
// chunk is, the path's own next cell is taken.  nk, the first index above i with a keep flag, moves on only when i
// reaches it: the flags are scanned once along the path.  Occ is OccBits, the image k_grid_occ_bits packed (OccGrid, the
// doubles themselves, only in the measurement of DESIGN.md 28: -DRMPC_SHORTEN_READS_GRID).
template <bool kLds, class Occ>
__global__ __launch_bounds__(64) void k_grid_shorten(const Occ occ, int H, int W, int B,
                                                     const int *__restrict__ path, const int *__restrict__ len, int max_len,
                                                     int reach, const int *__restrict__ keep, int *__restrict__ out,
                                                     int *__restrict__ out_len, int *__restrict__ src) {
  extern __shared__ int lds_path[];
  const int b = blockIdx.x, lane = threadIdx.x, HW = H * W, L = len[b];
  if (L <= 0 || L > max_len) {
    if (lane == 0) out_len[b] = L <= 0 ? L : RMPC_GRID_TOO_LONG;
    return;
  }
  const int *const pg = path + (size_t)b * max_len;
  bool outside = false;
  for (int k = lane; k < L; k += 64) {
    const int c = pg[k];
    outside = outside || c < 0 || c >= HW;
    if (kLds) lds_path[k] = c;
  }
  if (__ballot(outside)) {                 // (the workgroup is this one wavefront)
    if (lane == 0) out_len[b] = RMPC_GRID_OUTSIDE;
    return;
  }
  if (kLds) __syncthreads();               // the LDS copy before its reads
  const int *const p = kLds ? lds_path : pg;
  const int *const kp = keep ? keep + (size_t)b * max_len : nullptr;
  int *const o = out + (size_t)b * max_len;
  int *const s = src ? src + (size_t)b * max_len : nullptr;
  const int window = reach == 0 || reach > L - 1 ? L - 1 : reach;
  if (lane == 0) { o[0] = p[0]; if (s) s[0] = 0; }
  int i = 0, n = 1, nk = kp ? 0 : L;
  while (i < L - 1) {
    if (nk <= i) {                         // the first flag above i, L when there is none
      nk = L;
      for (int k0 = i + 1; k0 < L; k0 += 64) {
        const unsigned long long m = __ballot(k0 + lane < L && kp[k0 + lane] != 0);
        if (m) { nk = k0 + __builtin_ctzll(m); break; }
      }
    }
    int hi = i + window < L - 1 ? i + window : L - 1;
    hi = nk < hi ? nk : hi;
    const int a = p[i], ar = a / W, ac = a - ar * W;
    int j = i + 1;
    for (int top = hi; top >= i + 2; ) {
      const int base = top - 63 > i + 2 ? top - 63 : i + 2, k = base + lane;
      bool see = false;
      if (k <= top) {
        const int c = p[k], cr = c / W;
        see = grid_visible(occ, ar, ac, cr, c - cr * W);
      }
      const unsigned long long m = __ballot(see);
      if (m) { j = base + 63 - __builtin_clzll(m); break; }
      top = base - 1;
    }
    if (lane == 0) { o[n] = p[j]; if (s) s[n] = j; }
    n++;
    i = j;
  }
  if (lane == 0) out_len[b] = n;
}

// One wavefront per robot, kFollowWaves robots per workgroup, lane l the candidate i + 1 + l.  It reads the doubles: the
// map may change every control step and the walks are a few cells long.
__global__ __launch_bounds__(64 * kFollowWaves) void k_follow_visible(const int *__restrict__ path, const int *__restrict__ len,
                                                                      int max_len, int *__restrict__ idx,
                                                                      const double *__restrict__ pos, int stride, int B, int H,
                                                                      int W, const double *__restrict__ grid,
                                                                      double occ_threshold, double x0, double y0, double cell,
                                                                      int reach, double look_ahead, double *__restrict__ goal,
                                                                      int *__restrict__ blocked) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, b = blockIdx.x * kFollowWaves + (threadIdx.x >> 6);
  if (b >= B) return;
  const int L = len[b];
  if (L <= 0) return;
  const int *const p = path + (size_t)b * max_len;
  int i = idx[b];
  i = i < 0 ? 0 : (i >= L ? L - 1 : i);
  const double px = pos[(size_t)b * stride], py = pos[(size_t)b * stride + 1];
  const double fc = rint((px - x0) / cell), fr = rint((py - y0) / cell);
  const bool inside = fc >= 0.0 && fc < (double)W && fr >= 0.0 && fr < (double)H;
  const int last = i + reach < L - 1 ? i + reach : L - 1;
  auto qualifies = [&](int k) {
    const int c = p[k];
    const double cx = x0 + (double)(c % W) * cell, cy = y0 + (double)(c / W) * cell;
    const double dx = cx - px, dy = cy - py;
    return c >= 0 && c < H * W && sqrt(dx * dx + dy * dy) <= look_ahead &&
           grid_visible(OccGrid{grid, W, occ_threshold}, (int)fr, (int)fc, c / W, c % W);
  };
  // the up to 64 candidates above i at once; p [i] itself only when none of them qualifies
  const unsigned long long m = __ballot(inside && i + 1 + lane <= last && qualifies(i + 1 + lane));
  if (lane != 0) return;
  const bool any = m || (inside && qualifies(i));
  const int j = m ? i + 64 - __builtin_clzll(m) : i, c = p[j];
  idx[b] = j;
  goal[(size_t)b * 3] = x0 + (double)(c % W) * cell;
  goal[(size_t)b * 3 + 1] = y0 + (double)(c / W) * cell;
  goal[(size_t)b * 3 + 2] = 0.0;
  if (blocked) blocked[b] = any ? 0 : 1;
}

}  // namespace rmpc
