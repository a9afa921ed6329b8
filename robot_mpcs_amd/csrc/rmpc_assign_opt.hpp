// rmpc_assign_opt.hpp -- minimum-cost assignment of robots to targets on the device (include/rmpc_assign_opt.h,
// DESIGN.md 23), included by rmpc_world.hip beside rmpc_assign.hpp.  Two kernels: k_assign_quantise turns the fp64 costs
// of all problems into the oriented int32 matrices of the workspace over the whole chip, k_assign_optimal runs the
// shortest augmenting paths of the header, one workgroup per problem.  Every choice is a minimum of integers under a
// strict total order, so no result depends on the order in which lanes meet.  Contraction is off, as in rmpc_assign.hpp.

namespace rmpc {

constexpr int kAssignOptMaxQ = RMPC_ASSIGN_OPT_MAX_Q;
constexpr int kAssignOptKeyBits = 13;                        // the column (from 1, <= 4096) in the low bits of the key
constexpr long long kAssignOptBig = 1ll << 62;
static_assert(kAssignMaxRobots < (1 << kAssignOptKeyBits) && kAssignMaxTargets <= 1024 &&
              (long long)kAssignMaxTargets * kAssignOptMaxQ + 1 <= INT_MAX,
              "k_assign_optimal: (minv, column) in one 64-bit key, P in an int32");

// the workspace: Qmax [G] int32 (padded to 256 bytes), then the matrices [G][m][n] int32
__host__ __device__ inline long long assign_opt_matrix_offset(int G) { return ((long long)G * 4 + 255) / 256 * 256; }

// The word of the lane OFF away in the butterfly of a whole wavefront, by vector moves inside the SIMD (the controls of
// lane_xchg in rmpc_inst.hpp): 32 and 16 by v_permlane32_swap / v_permlane16_swap of the word with a copy of itself, 8
// by row_ror:8, 2 and 1 by quad permutations, all exactly lane ^ OFF; 4 by row_ror:4, which is lane ^ 4 or that lane's
// level-8 partner -- behind the level-8 step both hold the same minimum.  All 64 lanes must be active.
template <int OFF>
__device__ __forceinline__ unsigned assign_opt_xchg(const unsigned v) {
  static_assert(OFF == 32 || OFF == 16 || OFF == 8 || OFF == 4 || OFF == 2 || OFF == 1, "a butterfly level of a wavefront");
  if constexpr (OFF >= 16) {
    const bool odd = (threadIdx.x & OFF) != 0;               // (workgroups are whole wavefronts)
    if constexpr (OFF == 32) {
      const auto a = __builtin_amdgcn_permlane32_swap(v, v, false, false);
      return odd ? a[0] : a[1];
    } else {
      const auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false);
      return odd ? a[0] : a[1];
    }
  }
  else if constexpr (OFF == 8) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, true);   // row_ror:8
  else if constexpr (OFF == 4) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xF, 0xF, true);   // row_ror:4
  else if constexpr (OFF == 2) return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);    // quad_perm [2, 3, 0, 1]
  else return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);                            // quad_perm [1, 0, 3, 2]
}
template <int OFF>
__device__ __forceinline__ unsigned long long assign_opt_min_level(const unsigned long long k) {
  const unsigned lo = assign_opt_xchg<OFF>((unsigned)k), hi = assign_opt_xchg<OFF>((unsigned)(k >> 32));
  const unsigned long long o = ((unsigned long long)hi << 32) | lo;
  return o < k ? o : k;
}
// the least key of the wavefront, in every lane
__device__ __forceinline__ unsigned long long assign_opt_wave_min(unsigned long long k) {
  k = assign_opt_min_level<32>(k);
  k = assign_opt_min_level<16>(k);
  k = assign_opt_min_level<8>(k);
  k = assign_opt_min_level<4>(k);
  k = assign_opt_min_level<2>(k);
  return assign_opt_min_level<1>(k);
}
template <int OFF>
__device__ __forceinline__ int assign_opt_max_level(const int q) {
  const int o = (int)assign_opt_xchg<OFF>((unsigned)q);
  return o > q ? o : q;
}
// the greatest value of the wavefront, in every lane
__device__ __forceinline__ int assign_opt_wave_max(int q) {
  q = assign_opt_max_level<32>(q);
  q = assign_opt_max_level<16>(q);
  q = assign_opt_max_level<8>(q);
  q = assign_opt_max_level<4>(q);
  q = assign_opt_max_level<2>(q);
  return assign_opt_max_level<1>(q);
}

// One lane per entry (g, i, j) of the oriented matrices, total = G m n of them: Q [g][i][j] = q of the pair (robot i,
// target j) when B <= T, of (robot j, target i) otherwise, or -1 when the pair is not takeable (the solver's row load
// puts P there); qmax [g], zero before the launch, takes the greatest q of problem g.  The writes are consecutive in
// every case, the reads when B <= T.  A wavefront sends one atomic for the problem of its first lane and one per lane
// that lies in another problem.
__global__ __launch_bounds__(256) void k_assign_quantise(int B, int T, long long total, const double *__restrict__ cost,
                                                         double scale, int *__restrict__ qmax, int *__restrict__ Q) {
#pragma clang fp contract(off)
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int m = B <= T ? B : T, n = B <= T ? T : B;
  int g = 0, q = -1;
  if (idx < total) {
    const int mn = m * n;                                    // B T <= G B T <= INT_MAX
    g = (int)(idx / mn);
    const int rem = (int)(idx - (long long)g * mn);
    const int i = rem / n, j = rem - i * n;
    const double c = cost[B <= T ? idx : (long long)g * mn + (long long)j * T + i];
    const double r = __builtin_rint(c * scale);
    if (c >= 0.0 && c < __builtin_inf() && r <= (double)kAssignOptMaxQ) q = (int)r;
    Q[idx] = q;
  }
  const int g0 = __builtin_amdgcn_readfirstlane(g);          // (a wave without an entry has g = 0, q = -1 in every lane)
  const int best = assign_opt_wave_max(g == g0 ? q : -1);
  if ((threadIdx.x & 63) == 0 && best > 0) atomicMax(&qmax[g0], best);
  if (g != g0 && q > 0) atomicMax(&qmax[g], q);
}

// The loop of include/rmpc_assign_opt.h for problem blockIdx.x, with blockDim.x = min(1024, n rounded up to whole
// wavefronts) threads.  Thread t owns the columns c = t + k blockDim.x (from 0; the header's j = c + 1), k < CPT: v,
// minv, used and the column's row p of those live in its registers.  u [0..m], p [0..n] and way [1..n] live in LDS:
// s_way [j] is written by the column's thread only, s_p changes only between two rows' searches, and the potential of
// a used column's row is touched by that column's thread only (the root's row by thread 0), so nothing races.
//
// A step: the row's potential from LDS (a broadcast read), one coalesced load of the row of Q, the columns' update, the
// argmin of the key minv << 13 | j -- a DPP reduction inside each wave, then the waves' keys through LDS slots that
// alternate between steps, with the step's one workgroup barrier --, the dual update, and the next row s_p [j1].  The
// row read at the top of a step belongs to a column that was unused in the step before, so its potential was last
// written before that step's barrier.  With MAXT = 64 the workgroup is one wave: the keys meet in registers and the
// barriers around the augmentation are no instruction at all.  The path is walked backwards by thread 0 in LDS.
template <int MAXT, int CPT>
__global__ __launch_bounds__(MAXT) void k_assign_optimal(int B, int T, const int *__restrict__ qmax,
                                                         const int *__restrict__ Qall, int *__restrict__ assign,
                                                         long long *__restrict__ total_out, int *__restrict__ count_out,
                                                         int *__restrict__ steps_out) {
  constexpr int COLS = MAXT * CPT, ROWS = COLS < kAssignMaxTargets ? COLS : kAssignMaxTargets;
  static_assert(MAXT % 64 == 0 && MAXT <= 1024 && COLS <= kAssignMaxRobots && (CPT == 1 || MAXT == 1024), "k_assign_optimal");
  __shared__ long long s_u[ROWS + 1];
  __shared__ int s_p[COLS + 1], s_way[COLS + 1];
  __shared__ unsigned long long s_key[2][MAXT / 64];
  __shared__ unsigned long long s_total;
  __shared__ int s_count;
  const int g = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, nw = nt >> 6;
  const bool by_robot = B <= T;                              // the rows are the robots
  const int m = by_robot ? B : T, n = by_robot ? T : B;
  const int *const Q = Qall + (size_t)g * m * n;
  const long long P = (long long)m * qmax[g] + 1;
  long long v[CPT], minv[CPT];
  int p[CPT];
  bool used[CPT];
#pragma unroll
  for (int k = 0; k < CPT; k++) {
    const int c = tid + k * nt;
    v[k] = 0; p[k] = 0;
    if (c < n) s_p[c + 1] = 0;
  }
  for (int i = tid; i <= m; i += nt) s_u[i] = 0;
  if (tid == 0) { s_total = 0; s_count = 0; }
  __syncthreads();
  int steps = 0, par = 0;
  for (int i = 1; i <= m; i++) {
#pragma unroll
    for (int k = 0; k < CPT; k++) { minv[k] = kAssignOptBig; used[k] = false; }
    int j0 = 0, i0 = i;
    do {
      const long long ui0 = s_u[i0];
      const int *const row = Q + (size_t)(i0 - 1) * n;
      unsigned long long key = ~0ull;
#pragma unroll
      for (int k = 0; k < CPT; k++) {
        const int c = tid + k * nt;
        if (c < n && !used[k]) {
          const int q = row[c];
          const long long cur = (q < 0 ? P : (long long)q) - ui0 - v[k];
          if (cur < minv[k]) { minv[k] = cur; s_way[c + 1] = j0; }
          const unsigned long long mine = ((unsigned long long)minv[k] << kAssignOptKeyBits) | (unsigned)(c + 1);
          key = mine < key ? mine : key;                     // columns ascend within a thread, and the key holds the column
        }
      }
      key = assign_opt_wave_min(key);
      if constexpr (MAXT > 64) {
        if ((tid & 63) == 0) s_key[par][tid >> 6] = key;
        __syncthreads();
        for (int w = 0; w < nw; w++) {
          const unsigned long long o = s_key[par][w];
          key = o < key ? o : key;
        }
        par ^= 1;
      }
      const long long delta = (long long)(key >> kAssignOptKeyBits);
      const int j1 = (int)(key & ((1u << kAssignOptKeyBits) - 1));       // in [1, n]: row i0 always has an unused column
#pragma unroll
      for (int k = 0; k < CPT; k++) {
        const int c = tid + k * nt;
        if (c < n) {
          if (used[k]) { s_u[p[k]] += delta; v[k] -= delta; }
          else minv[k] -= delta;
          if (c + 1 == j1) used[k] = true;
        }
      }
      if (tid == 0) s_u[i] += delta;                         // the root's row
      steps++;
      j0 = j1;
      i0 = s_p[j1];
    } while (i0 != 0);
    __syncthreads();
    if (tid == 0) {
      s_p[0] = i;
      int j = j0;
      do {
        const int jw = s_way[j];
        s_p[j] = s_p[jw];
        j = jw;
      } while (j != 0);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CPT; k++) {
      const int c = tid + k * nt;
      if (c < n) p[k] = s_p[c + 1];
    }
  }
  // the report: every row holds a column; a robot's pair counts when it is takeable
  long long tot = 0;
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < CPT; k++) {
    const int c = tid + k * nt;
    if (c >= n) continue;
    const int q = p[k] ? Q[(size_t)(p[k] - 1) * n + c] : -1;
    if (q >= 0) { tot += q; cnt++; }
    if (by_robot) {
      if (p[k]) assign[(size_t)g * B + p[k] - 1] = q >= 0 ? c : -1;
    } else {
      assign[(size_t)g * B + c] = q >= 0 ? p[k] - 1 : -1;
    }
  }
  if (cnt) { atomicAdd(&s_total, (unsigned long long)tot); atomicAdd(&s_count, cnt); }
  __syncthreads();
  if (tid == 0) {
    if (total_out) total_out[g] = (long long)s_total;
    if (count_out) count_out[g] = s_count;
    if (steps_out) steps_out[g] = steps;
  }
}

}  // namespace rmpc
