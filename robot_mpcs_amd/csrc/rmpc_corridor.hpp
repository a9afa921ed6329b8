// rmpc_corridor.hpp -- safe corridors from the map (include/rmpc_corridor.h), included by
// rmpc_world.hip: k_occ_row_sums and k_occ_col_sums build the occupancy's summed-area table once per map,
// k_grid_corridor grows one rectangle of free cells per (robot, stage) seed on it and writes its four faces as
// half-planes.  The rule is the header's.  Everything that decides is integer arithmetic; contraction is off where
// doubles are formed, so the planes are bitwise a plain restatement.  Every loop is bounded (by W, by H, by reach + 1
// rounds), no workgroup waits for another and there are no atomics.

namespace rmpc {

constexpr int kSumsRowWaves = 4;           // rows per workgroup of k_occ_row_sums, a wavefront each
constexpr int kSumsColBatch = 8;           // rows whose loads k_occ_col_sums issues before it adds them

// Row prefix sums: one wavefront per row, 64 cells per step.  A lane's inclusive prefix within the step is the
// popcount of the ballot below and at its lane; the carry is the popcount of the ballots before.  Writes row r + 1 of
// S, its column 0 included.
__global__ __launch_bounds__(64 * kSumsRowWaves) void k_occ_row_sums(const double *__restrict__ grid, int H, int W,
                                                                     double occ_threshold, int *__restrict__ sums) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * kSumsRowWaves + (threadIdx.x >> 6);
  if (r >= H) return;                      // (the whole wavefront)
  const double *const g = grid + (size_t)r * W;
  int *const s = sums + (size_t)(r + 1) * (W + 1);
  if (lane == 0) s[0] = 0;
  const unsigned long long below = ~0ull >> (63 - lane);      // the lanes up to and including this one
  int carry = 0;
  for (int c0 = 0; c0 < W; c0 += 64) {
    const int c = c0 + lane;
    const bool o = c < W && !(g[c] < occ_threshold);
    const unsigned long long m = __ballot(o);
    if (c < W) s[c + 1] = carry + __popcll(m & below);
    carry += __popcll(m);
  }
}

// Column prefix sums over the rows k_occ_row_sums wrote: one thread per column of S, a wavefront's loads of a row
// coalesce.  Writes row 0 (zeros) and adds down the rows, kSumsColBatch rows' loads in flight at a time.
__global__ __launch_bounds__(256) void k_occ_col_sums(int H, int W, int *__restrict__ sums) {
  const int j = blockIdx.x * 256 + threadIdx.x, Ws = W + 1;
  if (j >= Ws) return;
  sums[j] = 0;
  int acc = 0, r = 1;
  for (; r + kSumsColBatch <= H + 1; r += kSumsColBatch) {
    int v[kSumsColBatch];
#pragma unroll
    for (int k = 0; k < kSumsColBatch; k++) v[k] = sums[(size_t)(r + k) * Ws + j];
#pragma unroll
    for (int k = 0; k < kSumsColBatch; k++) {
      acc += v[k];
      sums[(size_t)(r + k) * Ws + j] = acc;
    }
  }
  for (; r <= H; r++) {
    acc += sums[(size_t)r * Ws + j];
    sums[(size_t)r * Ws + j] = acc;
  }
}

// the header's box count on S (row stride Ws = W + 1): rows ra .. rb, columns ca .. cb, all inside the map
__device__ __forceinline__ int occ_count(const int *__restrict__ S, int Ws, int ra, int rb, int ca, int cb) {
  return S[(rb + 1) * Ws + cb + 1] - S[ra * Ws + cb + 1] - S[(rb + 1) * Ws + ca] + S[ra * Ws + ca];
}

// One thread per seed.  A direction whose line was refused is not tried again: the rectangle only grows, so the line
// would be refused in every later round (the header's argument for reach + 1 rounds); what is written is the header's
// rule.
__global__ __launch_bounds__(256) void k_grid_corridor(const int *__restrict__ S, int H, int W, double x0, double y0, double cell,
                                                       int n, const double *__restrict__ points, int reach, int nobst,
                                                       int slot0, double *__restrict__ planes, int *__restrict__ rect,
                                                       int *__restrict__ status) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const double s0 = points[(size_t)t * 3], s1 = points[(size_t)t * 3 + 1], s2 = points[(size_t)t * 3 + 2];
  const double fc = rint((s0 - x0) / cell), fr = rint((s1 - y0) / cell);
  const int Ws = W + 1;
  double *const o = planes + ((size_t)t * nobst + slot0) * 4;
  int st = -1, r = 0, c = 0;
  if (fc >= 0.0 && fc < (double)W && fr >= 0.0 && fr < (double)H) {
    r = (int)fr;
    c = (int)fc;
    st = occ_count(S, Ws, r, r, c, c) != 0 ? 0 : 1;
  }
  if (status) status[t] = st;
  if (st <= 0) {
    // k_fsd's dummy plane, HalfPlane(seed + (20, 20, 0), seed): normal = seed - point
    const double p0 = s0 + 20.0, p1 = s1 + 20.0, p2 = s2 + 0.0;
    const double n0 = s0 - p0, n1 = s1 - p1, n2 = s2 - p2;
    const double d = -((n0 * p0 + n1 * p1) + n2 * p2);
    for (int k = 0; k < 4; k++) { o[4 * k] = n0; o[4 * k + 1] = n1; o[4 * k + 2] = n2; o[4 * k + 3] = d; }
    if (rect) { rect[4 * t] = -1; rect[4 * t + 1] = -1; rect[4 * t + 2] = -1; rect[4 * t + 3] = -1; }
    return;
  }
  int r0 = r, r1 = r, c0 = c, c1 = c;
  bool east = true, north = true, west = true, south = true;      // +col, +row, -col, -row can still advance
  for (int round = 0; round <= reach && (east || north || west || south); round++) {
    if (east && (east = c1 + 1 < W && c1 + 1 - c <= reach && occ_count(S, Ws, r0, r1, c1 + 1, c1 + 1) == 0)) c1++;
    if (north && (north = r1 + 1 < H && r1 + 1 - r <= reach && occ_count(S, Ws, r1 + 1, r1 + 1, c0, c1) == 0)) r1++;
    if (west && (west = c0 - 1 >= 0 && c - (c0 - 1) <= reach && occ_count(S, Ws, r0, r1, c0 - 1, c0 - 1) == 0)) c0--;
    if (south && (south = r0 - 1 >= 0 && r - (r0 - 1) <= reach && occ_count(S, Ws, r0 - 1, r0 - 1, c0, c1) == 0)) r0--;
  }
  const double xlo = x0 + ((double)c0 - 0.5) * cell, xhi = x0 + ((double)c1 + 0.5) * cell;
  const double ylo = y0 + ((double)r0 - 0.5) * cell, yhi = y0 + ((double)r1 + 0.5) * cell;
  o[0] = 1.0;   o[1] = 0.0;   o[2] = 0.0;  o[3] = -xlo;
  o[4] = -1.0;  o[5] = 0.0;   o[6] = 0.0;  o[7] = xhi;
  o[8] = 0.0;   o[9] = 1.0;   o[10] = 0.0; o[11] = -ylo;
  o[12] = 0.0;  o[13] = -1.0; o[14] = 0.0; o[15] = yhi;
  if (rect) { rect[4 * t] = r0; rect[4 * t + 1] = r1; rect[4 * t + 2] = c0; rect[4 * t + 3] = c1; }
}

}  // namespace rmpc
