// rmpc_host.hip -- the host side of the library (handle, descriptor checks, row tables, generated-view matching,
// workspace carving, the launch loop, the C ABI) and the kernels that do not depend on a kernel variant.  It reaches
// the kernels of a variant through the handle's entry of the variant table (VariantOps, rmpc_host.hpp), which the
// units built from rmpc_variants.hip fill while the library loads.
#include "rmpc_host.hpp"

namespace rmpc {

// ===========================================================================
// pack / unpack: instance-major ABI layout <-> batch-minor SoA (LDS transpose)
// ===========================================================================
// in[b][c], c = k*inner + j  ->  out[(j*N + k)*Bp + b]
__global__ __launch_bounds__(256) void k_pack(const double *__restrict__ in, double *__restrict__ out, int B,
                                              int C, int inner, int N, int Bp) {
  __shared__ double tile[64][65];
  const int b0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  // unconditional requests with clamped indices, all issued before the first LDS store (a branch around a
  // load makes the compiler wait for each element separately)
  double v[16];
#pragma unroll
  for (int u = 0; u < 16; u++) {
    const int r = ty + 4 * u;
    const int b = b0 + r < B ? b0 + r : B - 1, c = c0 + tx < C ? c0 + tx : C - 1;
    v[u] = in[(size_t)b * C + c];
  }
#pragma unroll
  for (int u = 0; u < 16; u++) tile[ty + 4 * u][tx] = v[u];
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    int c = c0 + r, b = b0 + tx;
    if (c < C && b < B) {
      int k = c / inner, j = c - k * inner;
      out[((size_t)j * N + k) * Bp + b] = tile[tx][r];
    }
  }
}

__global__ __launch_bounds__(256) void k_init(Ws W, const double *__restrict__ xinit, int B, int nx, double mu0, int warm) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  for (int j = 0; j < nx; j++) W.z[0][IDX(j, 0, b)] = xinit[(size_t)b * nx + j];
  W.status[b] = ST_ACTIVE;
  W.act_idx[b] = b;
  if (b == 0) *W.n_act = B;
  W.iters[b] = 0;
  W.ls[b] = 0;
  W.cur[b] = 0;
  W.newstep[b] = 0;
  W.amin_p[b] = (unsigned long long)__double_as_longlong(1.0);
  W.amin_d[b] = (unsigned long long)__double_as_longlong(1.0);
  W.redo[b] = 0; W.force_gn[b] = 0; W.gn_sticky[b] = 0; W.curv_fail[b] = 0; W.usedc[b] = 0; W.stall[b] = 0;
  W.curv_skip[b] = 0; W.curv_back[b] = 0;
  W.small_steps[b] = 0; W.mu_hold[b] = 0.0;
  W.theta_mem[b] = 1.0; W.theta_c[b] = 1.0; W.theta_clean[b] = 0; W.theta_retry[b] = 0;
  W.ls0[b] = 0; W.lsst[b] = 0;
  W.mu[b] = warm ? warm_mu(W.wmu[b], mu0) : mu0;
  W.rho[b] = 0.0;
  W.phi0[b] = 0.0;
  W.Dd[b] = 0.0;
  W.fcur[b] = 0.0;
  W.thcur[b] = 0.0;
  W.logcur[b] = 0.0;
  W.res_stat[b] = 0.0; W.res_eq[b] = 0.0; W.res_ineq[b] = 0.0; W.res_comp[b] = 0.0; W.obj[b] = 0.0;
}

// z (current buffer of each instance) -> z_out[b][k][v]; stats
__global__ __launch_bounds__(256) void k_unpack(Ws W, double *__restrict__ zout, int *__restrict__ exitflag,
                                                int *__restrict__ iters, double *__restrict__ kkt,
                                                double *__restrict__ obj, int B, int nv,
                                                const int *__restrict__ orig) {
  // orig != nullptr: W is the compact workspace, column b belongs to instance orig[b] of the batch
  __shared__ double tile[64][65];
  const int N = W.N;
  const int C = N * nv;
  const int b0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  {
    const int b = b0 + tx < B ? b0 + tx : B - 1;   // clamped: the requests stay unconditional
    const double *__restrict__ zb = W.z[W.cur[b]];
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const int c = c0 + ty + 4 * u < C ? c0 + ty + 4 * u : C - 1;
      const int k = c / nv, j = c - k * nv;
      v[u] = zb[IDX(j, k, b)];
    }
#pragma unroll
    for (int u = 0; u < 16; u++) tile[ty + 4 * u][tx] = v[u];
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    int b = b0 + r, c = c0 + tx;
    if (b < B && c < C) zout[(size_t)(orig ? orig[b] : b) * C + c] = tile[tx][r];
  }
  if (blockIdx.y == 0 && threadIdx.x < 64) {
    int b = b0 + threadIdx.x;
    if (b < B) {
      const int ob = orig ? orig[b] : b;
      int st = W.status[b];
      exitflag[ob] = (st == ST_ACTIVE) ? 0 : st;
      iters[ob] = W.iters[b];
      double r = fmax(fmax(W.res_stat[b], W.res_eq[b]), fmax(W.res_ineq[b], W.res_comp[b]));
      kkt[ob] = r;
      obj[ob] = W.obj[b];
    }
  }
}

// Multipliers of the finished solve -> the warm-start arrays of the batch's workspace D (W may be the compact
// workspace: column b then belongs to instance orig[b]).  One lane per (column, stage).
// d[j * ds] = s[j * ss], j < cnt, eight requests in flight (source and destination never alias: the copies below are
// chains of dependent latencies otherwise -- 50 us for the arm's multipliers, 105 us for a migration of 128 instances)
__device__ __forceinline__ void copy_strided(double *__restrict__ d, const double *__restrict__ s, const int cnt, const size_t ds,
                                             const size_t ss) {
  int j = 0;
  for (; j + 8 <= cnt; j += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = s[(size_t)(j + u) * ss];
#pragma unroll
    for (int u = 0; u < 8; u++) d[(size_t)(j + u) * ds] = v[u];
  }
  for (; j < cnt; j++) d[(size_t)j * ds] = s[(size_t)j * ss];
}
__device__ __forceinline__ void fill_strided(double *__restrict__ d, const double val, const int cnt, const size_t ds) {
  for (int j = 0; j < cnt; j++) d[(size_t)j * ds] = val;
}

__global__ __launch_bounds__(256) void k_save_duals(const Ws W, const Ws D, int B, int m, int nx, const int *__restrict__ orig,
                                                    double mu0) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int b = gid % W.Bp, k = gid / W.Bp;
  if (b >= B || k >= W.N) return;
  const int cur = W.cur[b];
  const int ob = orig ? orig[b] : b;
  // a failed solve leaves nothing to start from: zero multipliers and mu0 (the warm start then degenerates to
  // lambda = mu0 / t, nu = 0)
  const int st = W.status[b];
  const double mu = W.mu[b];
  const bool ok = (st == ST_ACTIVE || st >= 0) && isfinite(mu) && mu > 0.0;
  double *const dl = D.wlam + (size_t)k * D.Bp + ob, *const dn = D.wnu + (size_t)k * D.Bp + ob;
  const size_t ds = (size_t)D.N * D.Bp, ss = (size_t)W.N * W.Bp;
  if (ok) {
    copy_strided(dl, W.lam[cur] + (size_t)k * W.Bp + b, m, ds, ss);
    copy_strided(dn, W.nu[cur] + (size_t)k * W.Bp + b, nx, ds, ss);
  } else {
    fill_strided(dl, 0.0, m, ds);
    fill_strided(dn, 0.0, nx, ds);
  }
  if (k == 0) D.wmu[ob] = ok ? mu : mu0;
}

// ===========================================================================
// k_compact: ordered list of the instances that are still iterating.  All pass
// kernels index their lanes through it, so wavefronts beyond the list exit at
// once and the passes of the iteration tail touch a few wavefronts only.
// ===========================================================================
__global__ __launch_bounds__(1024) void k_compact(Ws W, int B, int pass) {
  __shared__ int sums[1024];
  const int tid = threadIdx.x;
  // (passes enqueued without a host look, rmpc_set_pass_budget: once nothing iterates any more the remaining passes
  //  are empty launches -- this one too; active_hist was zeroed before the solve)
  if (pass > 0 && *W.n_act == 0) return;
  const int per = (B + 1023) / 1024;
  const int lo = tid * per, hi = (lo + per < B) ? lo + per : B;
  int cnt = 0;
  for (int b = lo; b < hi; b++) cnt += (W.status[b] == ST_ACTIVE);
  sums[tid] = cnt;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = (tid >= off) ? sums[tid - off] : 0;
    __syncthreads();
    sums[tid] += v;
    __syncthreads();
  }
  const int total = sums[1023];
  // while most instances are still iterating the identity list keeps every access coalesced
  const bool dense = (total * kDenseDiv > B);
  int base = dense ? lo : sums[tid] - cnt;
  for (int b = lo; b < hi; b++)
    if (dense || W.status[b] == ST_ACTIVE) W.act_idx[base++] = b;
  if (tid == 1023) {
    *W.n_act = dense ? B : total;
    W.active_hist[pass] = total;
  }
}

// The same list from ONE wavefront (batches up to kCompactWaveMax instances).  With other handles' kernels on the chip
// every SIMD holds a long-lived 512-register wavefront, and the 16-wavefront block above waits until a whole compute
// unit has drained: in a trace of four arm batches in flight k_compact took 25 us on average (p90 93 us) for 5 us of
// work -- once per pass, on the critical path of its stream.  A single wavefront takes the first SIMD that frees.
// 64 instances per round (one coalesced request, ballot + popcount instead of a scan), eight rounds in flight.
constexpr int kCompactWaveMax = 8192;
__global__ __launch_bounds__(64) void k_compact_wave(Ws W, int B, int pass) {
  const int lane = threadIdx.x;
  if (pass > 0 && *W.n_act == 0) return;
  const int rounds = (B + 63) / 64;
  int total = 0;
  for (int r0 = 0; r0 < rounds; r0 += 8) {
    int st[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int b = (r0 + u) * 64 + lane;
      st[u] = W.status[b < B ? b : B - 1];
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int b = (r0 + u) * 64 + lane;
      total += __popcll(__ballot(b < B && st[u] == ST_ACTIVE));
    }
  }
  const bool dense = (total * kDenseDiv > B);
  const unsigned long long below = (1ull << lane) - 1ull;
  int base = 0;
  for (int r0 = 0; r0 < rounds; r0 += 8) {
    int st[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int b = (r0 + u) * 64 + lane;
      st[u] = W.status[b < B ? b : B - 1];
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int b = (r0 + u) * 64 + lane;
      const bool on = b < B && (dense || st[u] == ST_ACTIVE);
      const unsigned long long mk = __ballot(on);
      if (on) W.act_idx[base + __popcll(mk & below)] = b;
      base += __popcll(mk);
    }
  }
  if (lane == 0) {
    *W.n_act = dense ? B : total;
    W.active_hist[pass] = total;
  }
}

// ===========================================================================
// k_migrate: once few instances are left their whole iteration state moves to the
// dense columns 0..n-1 of a small second workspace.  Indexing scattered survivors
// through the list costs a 64-byte sector per 8-byte element (every pass then moves
// as many bytes as a full batch); one gather of that kind pays for itself in the
// next pass.  Runs between k_step and the next k_sweep: what crosses that boundary
// is the current iterate, the step, the parameters and the per-instance words.
// ===========================================================================
__global__ __launch_bounds__(64) void k_migrate(const Ws S, const Ws D, int n, int nv, int m, int nx, int npar, int nh,
                                                int njq) {
  const int li = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y;
  if (li >= n) return;
  const int b = S.act_idx[li];
  const int cur = S.cur[b];
  auto si = [&](int slot) { return ((size_t)slot * S.N + k) * S.Bp + b; };
  auto di = [&](int slot) { return ((size_t)slot * D.N + k) * D.Bp + li; };
  {
    const size_t ds = (size_t)D.N * D.Bp, ss = (size_t)S.N * S.Bp, d0 = di(0), s0 = si(0);
    copy_strided(D.z[0] + d0, S.z[cur] + s0, nv, ds, ss);
    copy_strided(D.dz + d0, S.dz + s0, nv, ds, ss);
    copy_strided(D.t[0] + d0, S.t[cur] + s0, m, ds, ss);
    copy_strided(D.lam[0] + d0, S.lam[cur] + s0, m, ds, ss);
    copy_strided(D.grow[0] + d0, S.grow[cur] + s0, nh, ds, ss);
    copy_strided(D.Jq[0] + d0, S.Jq[cur] + s0, njq, ds, ss);
    copy_strided(D.nu[0] + d0, S.nu[cur] + s0, nx, ds, ss);
    copy_strided(D.nunew + d0, S.nunew + s0, nx, ds, ss);
    copy_strided(D.p + d0, S.p + s0, npar, ds, ss);
  }
  D.gphi[di(0)] = S.gphi[si(0)];
  if (k == 0) {
    D.amin_p[li] = S.amin_p[b]; D.amin_d[li] = S.amin_d[b];
    D.mu[li] = S.mu[b]; D.rho[li] = S.rho[b]; D.phi0[li] = S.phi0[b]; D.Dd[li] = S.Dd[b];
    D.fcur[li] = S.fcur[b]; D.thcur[li] = S.thcur[b]; D.logcur[li] = S.logcur[b];
    D.res_stat[li] = S.res_stat[b]; D.res_eq[li] = S.res_eq[b]; D.res_ineq[li] = S.res_ineq[b];
    D.res_comp[li] = S.res_comp[b]; D.obj[li] = S.obj[b];
    D.status[li] = S.status[b]; D.iters[li] = S.iters[b]; D.ls[li] = S.ls[b]; D.newstep[li] = S.newstep[b];
    D.redo[li] = S.redo[b]; D.force_gn[li] = S.force_gn[b]; D.gn_sticky[li] = S.gn_sticky[b];
    D.curv_fail[li] = S.curv_fail[b]; D.usedc[li] = S.usedc[b]; D.stall[li] = S.stall[b];
    D.curv_skip[li] = S.curv_skip[b]; D.curv_back[li] = S.curv_back[b];
    D.small_steps[li] = S.small_steps[b]; D.mu_hold[li] = S.mu_hold[b];
    D.theta_mem[li] = S.theta_mem[b]; D.theta_c[li] = S.theta_c[b]; D.theta_clean[li] = S.theta_clean[b]; D.theta_retry[li] = S.theta_retry[b];
    D.ls0[li] = S.ls0[b]; D.lsst[li] = S.lsst[b];
    D.cur[li] = 0;
    D.orig[li] = b;
    D.act_idx[li] = li;
    if (li == 0) *D.n_act = n;
  }
}

// Launch order of a fused launch: the instances sorted by a key (the passes of their previous solve for a warm start,
// k_difficulty's estimate for a cold one), largest first (counting sort, one block; the order inside a bucket is
// whatever the atomics give -- it changes which instances share a wavefront, never what an instance computes).
// (NT = 64 for the order of a cold launch, which runs IN FRONT of the fused launch: with other handles' fused launches
//  on the chip every SIMD is held by one long-lived 512-register wavefront, and a block of several wavefronts would
//  wait until a whole compute unit has drained; a single wavefront takes the first SIMD that frees)
template <int NT>
static __global__ __launch_bounds__(NT) void k_order_t(const int *__restrict__ key, int *__restrict__ order, int B) {
  __shared__ int cnt[256];
  const int tid = threadIdx.x;
  for (int i = tid; i < 256; i += NT) cnt[i] = 0;
  __syncthreads();
  // (eight keys per lane and round: the requests of a round are in flight together -- one by one the single
  //  wavefront of the cold order spent 33 us on 4096 keys, most of it waiting for one key at a time)
  constexpr int U = 8;
  for (int b0 = tid; b0 < B; b0 += NT * U) {
    int kq[U];
#pragma unroll
    for (int u = 0; u < U; u++) { const int b = b0 + u * NT; kq[u] = key[b < B ? b : B - 1]; }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int kk = kq[u] < 0 ? 0 : (kq[u] > 255 ? 255 : kq[u]);
      if (b0 + u * NT < B) atomicAdd(&cnt[255 - kk], 1);
    }
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < 256; i++) { const int c = cnt[i]; cnt[i] = run; run += c; }
  }
  __syncthreads();
  for (int b0 = tid; b0 < B; b0 += NT * U) {
    int kq[U];
#pragma unroll
    for (int u = 0; u < U; u++) { const int b = b0 + u * NT; kq[u] = key[b < B ? b : B - 1]; }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int kk = kq[u] < 0 ? 0 : (kq[u] > 255 ? 255 : kq[u]);
      if (b0 + u * NT < B) order[atomicAdd(&cnt[255 - kk], 1)] = b0 + u * NT;
    }
  }
}

struct SceneDev {
  const double *goal, *r_body, *obst, *obst_dyn, *lower, *upper, *lower_u, *upper_u, *lower_vel, *upper_vel, *lin;
  double dyn_radius, w, wu, ws;
  double wconstr[RMPC_MAX_MODULES];
};
struct SceneOff {
  int r_body, obst, lin, lower, upper, lower_u, upper_u, lower_vel, upper_vel, wu, goal, wgoal, wconstr, ws;
  int n, nu, nobst, n_modules, npar, N;
  double dt;
};

// One lane per (instance, stage).  SOA = 0: ABI layout params[b][k][npar] (what
// MPCPlanner.reset() + set*() + updateDynamicObstacles() produce, mpcPlanner.py:83-210);
// SOA = 1: straight into the pass kernels' batch-minor parameter array; SOA = 2: into the fused kernel's
// per-instance layout.
template <int SOA>
__global__ __launch_bounds__(256) void k_scene(const SceneDev S, const SceneOff O, double *__restrict__ out, int B, int Bp) {
#pragma clang fp contract(off)
  const int gid = blockIdx.x * 256 + threadIdx.x;
  int b, k;
  if (SOA == 1) { b = gid % Bp; k = gid / Bp; } else { k = gid % O.N; b = gid / O.N; }
  if (b >= B || k >= O.N) return;
  auto put = [&](int off, double v) __attribute__((always_inline)) {
    if (SOA == 1) out[((size_t)off * O.N + k) * Bp + b] = v;
    else if (SOA == 2) out[((size_t)b * O.npar + off) * kFusedStages + k] = v;   // fused kernel: [instance][slot][32 stages]
    else out[((size_t)b * O.N + k) * O.npar + off] = v;
  };
  // reset(): zeros, then the broadcast weights (mpcPlanner.py:91-104)
  for (int j = 0; j < O.npar; j++) put(j, 0.0);
  if (O.wgoal >= 0) for (int j = 0; j < 3; j++) put(O.wgoal + j, S.w);
  for (int j = 0; j < O.nu; j++) put(O.wu + j, S.wu);
  if (O.ws >= 0) put(O.ws, S.ws);
  if (O.wconstr >= 0) for (int j = 0; j < O.n_modules; j++) put(O.wconstr + j, S.wconstr[j]);
  if (O.goal >= 0 && S.goal) for (int j = 0; j < 3; j++) put(O.goal + j, S.goal[(size_t)b * 3 + j]);
  if (O.r_body >= 0 && S.r_body) put(O.r_body, S.r_body[b]);
  if (O.obst >= 0) {
    if (S.obst_dyn) {
      // updateDynamicObstacles (mpcPlanner.py:144-161): c = pos + (vel*dt)*k + (0.5*(dt*k)^2)*acc
      const double kk = (double)k;
      for (int j = 0; j < O.nobst; j++) {
        const double *o = S.obst_dyn + ((size_t)b * O.nobst + j) * 9;
        for (int c = 0; c < 3; c++) {
          // every product and sum rounded separately (fp contraction is switched off for this
          // kernel): bit-identical to the reference's numpy expression pos + vel*dt*i + 0.5*(dt*i)**2*acc
          const double tk = O.dt * kk;
          const double lin = (o[3 + c] * O.dt) * kk;
          const double quad = (0.5 * (tk * tk)) * o[6 + c];
          put(O.obst + 4 * j + c, (o[c] + lin) + quad);
        }
        put(O.obst + 4 * j + 3, S.dyn_radius);
      }
    } else if (S.obst) {
      for (int j = 0; j < 4 * O.nobst; j++) put(O.obst + j, S.obst[(size_t)b * 4 * O.nobst + j]);
    } else {
      // no obstacles given: every slot is the reference's EmptyObstacle (position -100, radius -100;
      // mpcPlanner.py:18-26,127-133), as the host packer writes
      for (int j = 0; j < 4 * O.nobst; j++) put(O.obst + j, -100.0);
    }
  }
  if (O.lin >= 0 && S.lin)
    for (int j = 0; j < 4 * O.nobst; j++) put(O.lin + j, S.lin[((size_t)b * O.N + k) * 4 * O.nobst + j]);
  if (O.lower >= 0 && S.lower) for (int j = 0; j < O.n; j++) put(O.lower + j, S.lower[(size_t)b * O.n + j]);
  if (O.upper >= 0 && S.upper) for (int j = 0; j < O.n; j++) put(O.upper + j, S.upper[(size_t)b * O.n + j]);
  if (O.lower_u >= 0 && S.lower_u) for (int j = 0; j < O.nu; j++) put(O.lower_u + j, S.lower_u[(size_t)b * O.nu + j]);
  if (O.upper_u >= 0 && S.upper_u) for (int j = 0; j < O.nu; j++) put(O.upper_u + j, S.upper_u[(size_t)b * O.nu + j]);
  if (O.lower_vel >= 0 && S.lower_vel) for (int j = 0; j < 2; j++) put(O.lower_vel + j, S.lower_vel[(size_t)b * 2 + j]);
  if (O.upper_vel >= 0 && S.upper_vel) for (int j = 0; j < 2; j++) put(O.upper_vel + j, S.upper_vel[(size_t)b * 2 + j]);
}

// The environment of the moving obstacles between two control steps (what the examples' simulator does before the driver
// hands the planner ob[nx:], mpcPlanner.py:243-244): pos += vel dt + acc dt^2 / 2, vel += acc dt, one lane per
// (instance, obstacle); arena > 0: an obstacle that leaves [-arena, arena] in x or y comes back (velocity component
// mirrored), so that a loop that runs for hours keeps its obstacles.
static __global__ __launch_bounds__(256) void k_obst_advance(double *__restrict__ od, int n, double dt, double arena) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double *o = od + (size_t)i * 9;
  for (int c = 0; c < 3; c++) {
    double pos = o[c] + o[3 + c] * dt + 0.5 * o[6 + c] * dt * dt;
    double vel = o[3 + c] + o[6 + c] * dt;
    if (arena > 0.0 && c < 2) {
      if (pos > arena) { pos = 2.0 * arena - pos; vel = -vel; }
      else if (pos < -arena) { pos = -2.0 * arena - pos; vel = -vel; }
    }
    o[c] = pos; o[3 + c] = vel;
  }
}

// ===========================================================================
// Free-space decomposition: lidar point cloud -> at most K half-planes
// around a seed point, one lane per (instance, stage) seed.  Greedy rule of the reference
// (robotmpcs/utils/free_space_decomposition.py:79-97): the closest remaining point inside
// max_radius defines the plane through it with normal (seed - point); points on or behind the
// plane are discarded; unused slots get the dummy plane of asdict() (:110-114).  The sort of
// the reference is replaced by K arg-min sweeps over a keep-mask (P <= 64 points).
// ===========================================================================
__global__ __launch_bounds__(256) void k_fsd(const double *__restrict__ points, const double *__restrict__ seeds,
                                             double *__restrict__ out, int B, int N, int P, int K, double max_radius) {
#pragma clang fp contract(off)
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= B * N) return;
  const int b = gid / N;
  const double *pc = points + (size_t)b * P * 3;
  const double s0 = seeds[(size_t)gid * 3], s1 = seeds[(size_t)gid * 3 + 1], s2 = seeds[(size_t)gid * 3 + 2];
  double *o = out + (size_t)gid * K * 4;
  unsigned long long keep = 0ull;
  for (int i = 0; i < P; i++) {
    const double d0 = pc[3 * i] - s0, d1 = pc[3 * i + 1] - s1, d2 = pc[3 * i + 2] - s2;
    if (sqrt(d0 * d0 + d1 * d1 + d2 * d2) < max_radius) keep |= (1ull << i);
  }
  int nc = 0;
  while (keep && nc < K) {
    int best = -1;
    double bd = 0.0;
    for (int i = 0; i < P; i++)
      if (keep & (1ull << i)) {
        const double d0 = pc[3 * i] - s0, d1 = pc[3 * i + 1] - s1, d2 = pc[3 * i + 2] - s2;
        const double dd = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        if (best < 0 || dd < bd) { best = i; bd = dd; }
      }
    const double p0 = pc[3 * best], p1 = pc[3 * best + 1], p2 = pc[3 * best + 2];
    const double n0 = s0 - p0, n1 = s1 - p1, n2 = s2 - p2;
    const double c = -((n0 * p0 + n1 * p1) + n2 * p2);
    o[4 * nc] = n0; o[4 * nc + 1] = n1; o[4 * nc + 2] = n2; o[4 * nc + 3] = c;
    nc++;
    for (int i = 0; i < P; i++)
      if (keep & (1ull << i)) {
        const double v = ((n0 * pc[3 * i] + n1 * pc[3 * i + 1]) + n2 * pc[3 * i + 2]) + c;
        if (v <= 0.0) keep &= ~(1ull << i);
      }
  }
  for (; nc < K; nc++) {
    // HalfPlane(seed + (20, 20, 0), seed): normal = seed - point
    const double p0 = s0 + 20.0, p1 = s1 + 20.0, p2 = s2 + 0.0;
    const double n0 = s0 - p0, n1 = s1 - p1, n2 = s2 - p2;
    o[4 * nc] = n0; o[4 * nc + 1] = n1; o[4 * nc + 2] = n2; o[4 * nc + 3] = -((n0 * p0 + n1 * p1) + n2 * p2);
  }
}

}  // namespace rmpc

#include "rmpc_grid.hpp"
#include "rmpc_sense.hpp"

// ===========================================================================
// host side: handle, workspace, launch loop, C ABI
// ===========================================================================
static const char *kKernelNames[RMPC_NUM_KERNELS] = {"k_pack", "k_sweep", "k_riccati", "k_step", "k_unpack", "k_fused"};

// ---- variant table -------------------------------------------------------------------------------------------------
static std::vector<VariantOps> &variant_table() {
  static std::vector<VariantOps> t;
  return t;
}
void add_variant_ops(const VariantOps &v) { variant_table().push_back(v); }

// the runtime-table entry of the descriptor's variant, nullptr: the library holds none
static const VariantOps *variant_of(const rmpc_desc &d) {
  for (const VariantOps &v : variant_table())
    if (!v.matches && v.robot == d.robot && v.nq == d.n && v.ns == (d.ns ? 1 : 0)) return &v;
  return nullptr;
}

// the generated view whose tables equal the descriptor's, nullptr: none
static const VariantOps *find_spec(const rmpc_desc &d, const DevModel &M, const DevTables &T) {
  for (const VariantOps &v : variant_table())
    if (v.matches && v.matches(d, M, T)) return &v;
  return nullptr;
}

static std::string variant_list() {
  std::string s;
  for (const VariantOps &v : variant_table())
    if (!v.matches)
      s += (s.empty() ? "" : ", ") + (v.robot == RMPC_ROBOT_CHAIN ? "holonomic chain n = " + std::to_string(v.nq) : std::string("diff-drive base")) +
           (v.ns ? " with the slack variable" : "");
  return s;
}

// Row tables in device memory (DevTables): kinematic slots with their FK rows, and the
// single-variable rows grouped by variable.
static int build_tables(const rmpc_desc &d, const DevModel &M, DevTables &T, std::string &err) {
  memset(&T, 0, sizeof T);
  for (int s = 0; s < kMaxSlots; s++) { T.slot_fa[s] = -1; T.slot_fb[s] = -1; }
  for (int j = 0; j < RMPC_NV_MAX; j++)
    for (int u = 0; u < kVarRows; u++) { T.v_row[j][u] = -1; T.v_poff[j][u] = -1; T.v_mod[j][u] = -1; }
  auto slot_of = [&](int fa, int fb) -> int {
    for (int s = 0; s < T.nslots; s++)
      if (T.slot_fa[s] == fa && T.slot_fb[s] == fb) return s;
    if (T.nslots >= kMaxSlots) return -1;
    T.slot_fa[T.nslots] = fa; T.slot_fb[T.nslots] = fb;
    return T.nslots++;
  };
  if (d.has_goal && slot_of(d.end_frame, -1) != 0) { err = "slot table"; return -1; }
  // FK rows with their slots, then sorted by slot
  struct FkRow { int row, kind, obst, mod, first, idx, slot; };
  std::vector<FkRow> rows;
  for (int i = 0; i < M.nh; i++) {
    if (M.row_kind[i] == ROW_SINGLE) continue;
    const int fb = (M.row_kind[i] == ROW_SELF) ? M.row_b[i] : -1;
    const int s = slot_of(M.row_a[i], fb);
    if (s < 0) { err = "more than 4 distinct collision points (links / link pairs / end link)"; return -1; }
    rows.push_back({i, M.row_kind[i], M.row_kind[i] == ROW_SELF ? 0 : M.row_b[i], M.row_mod[i],
                    i == M.mod_row0[M.row_mod[i]] ? 1 : 0, M.row_fk[i], s});
  }
  if ((int)rows.size() > kMaxFkRows) { err = "too many distance rows"; return -1; }
  int r = 0;
  for (int s = 0; s < kMaxSlots; s++) {
    T.slot_row_begin[s] = r;
    for (const FkRow &fr : rows)
      if (fr.slot == s) {
        T.fk_row[r] = fr.row; T.fk_kind[r] = fr.kind; T.fk_obst[r] = fr.obst;
        T.fk_mod[r] = fr.mod; T.fk_first[r] = fr.first; T.fk_idx[r] = fr.idx;
        r++;
      }
  }
  T.slot_row_begin[kMaxSlots] = r;
  T.nfkrows = r;
  // single-variable rows
  auto add_var_row = [&](int var, int row, int sgn, int poff, double val, int soft, int mod, int firstrow) -> bool {
    for (int u = 0; u < kVarRows; u++)
      if (T.v_row[var][u] < 0) {
        T.v_row[var][u] = row; T.v_sgn[var][u] = sgn; T.v_poff[var][u] = poff;
        T.v_val[var][u] = val; T.v_soft[var][u] = soft; T.v_mod[var][u] = mod;
        T.v_first[var][u] = firstrow;
        return true;
      }
    return false;
  };
  bool ok = true;
  for (int i = 0; i < M.nh && ok; i++)
    if (M.row_kind[i] == ROW_SINGLE)
      ok = add_var_row(M.row_a[i], i, M.row_b[i], M.row_poff[i], 0.0, 1, M.row_mod[i], i == M.mod_row0[M.row_mod[i]] ? 1 : 0);
  int i = M.nh;
  for (int q = 0; q < M.nlb && ok; q++, i++) ok = add_var_row(M.lb_var[q], i, +1, -1, M.lb_val[q], 0, -1, 0);
  for (int q = 0; q < M.nub && ok; q++, i++) ok = add_var_row(M.ub_var[q], i, -1, -1, M.ub_val[q], 0, -1, 0);
  if (!ok) { err = "more than 4 limit / bound rows on one variable"; return -1; }
  // packed copies (fused arm kernel)
  for (int j = 0; j < RMPC_NV_MAX; j++)
    for (int u = 0; u < kVarRows; u++) {
      int w = 0;
      if (T.v_row[j][u] >= 0 && T.v_row[j][u] < 256 && T.v_poff[j][u] < 65536) {
        w = T.v_row[j][u] | (1 << 8) | ((T.v_sgn[j][u] < 0 ? 1 : 0) << 9) | ((T.v_first[j][u] ? 1 : 0) << 10) |
            ((T.v_poff[j][u] >= 0 ? 1 : 0) << 11) | ((T.v_mod[j][u] >= 0 ? T.v_mod[j][u] & 7 : 0) << 12) |
            ((T.v_poff[j][u] >= 0 ? T.v_poff[j][u] : 0) << 16);
      }
      T.v_desc[j][u] = w;
    }
  for (int q = 0; q < T.nfkrows; q++)
    T.fk_desc[q] = (T.fk_row[q] & 255) | ((T.fk_kind[q] & 3) << 8) | ((T.fk_obst[q] & 63) << 10) | ((T.fk_mod[q] & 7) << 16) |
                   ((T.fk_first[q] ? 1 : 0) << 19) | ((T.fk_idx[q] & 63) << 20);
  T.slot_rows_max = 0;
  for (int s = 0; s < kMaxSlots; s++)
    if (T.slot_row_begin[s + 1] - T.slot_row_begin[s] > T.slot_rows_max) T.slot_rows_max = T.slot_row_begin[s + 1] - T.slot_row_begin[s];
  return 0;
}

static int build_model(const rmpc_desc &d, DevModel &M, std::string &err) {
  memset(&M, 0, sizeof M);
  M.robot = d.robot; M.N = d.N; M.n = d.n; M.nx = d.nx; M.nu = d.nu; M.ns = d.ns;
  M.nv = d.nx + d.ns + d.nu; M.nw = d.ns + d.nu; M.npar = d.npar; M.dt = d.dt;
  if (d.N < 1 || d.N > 1000) { err = "horizon out of range"; return -1; }
  if (d.n_joints < 1 || d.n_joints > RMPC_MAX_JOINTS) { err = "n_joints out of range"; return -1; }
  if (d.ns != 0 && d.ns != 1) { err = "ns must be 0 or 1"; return -1; }
  if (d.robot == RMPC_ROBOT_CHAIN) {
    if (d.nx != 2 * d.n || d.nu != d.n) { err = "holonomic chain needs nx = 2n, nu = n"; return -1; }
    if (d.n_joints != d.n) { err = "chain with fixed joints between root and end link is not supported"; return -1; }
    for (int j = 0; j < d.n_joints; j++)
      if (d.joint_type[j] == RMPC_JOINT_FIXED || d.joint_dof[j] != j) { err = "chain joints must all be actuated, in order"; return -1; }
  } else if (d.robot == RMPC_ROBOT_DIFFDRIVE) {
    if (d.n != 3 || d.nx != 8 || d.nu != 2) { err = "diff-drive needs n = 3, nx = 8, nu = 2 (fk.n() == 0)"; return -1; }
    for (int j = 0; j < d.n_joints; j++)
      if (d.joint_type[j] != RMPC_JOINT_FIXED) { err = "diff-drive chain must consist of fixed joints"; return -1; }
  } else { err = "unknown robot kind"; return -1; }
  if (d.n_joints < 1 || d.n_joints > RMPC_MAX_JOINTS) { err = "n_joints out of range"; return -1; }
  if (M.nv > RMPC_NV_MAX) { err = "nvar too large"; return -1; }
  M.n_modules = d.n_modules; M.nobst = d.nobst; M.end_frame = d.end_frame; M.n_joints = d.n_joints;
  if (d.n_modules < 0 || d.n_modules > RMPC_MAX_MODULES) { err = "n_modules out of range"; return -1; }
  if (d.n_xrows < 0 || d.n_xrows > RMPC_MAX_XROWS) { err = "n_xrows out of range"; return -1; }
  for (int r = 0; r < d.n_xrows; r++)
    if (d.xrow_mod[r] < 0 || d.xrow_mod[r] >= d.n_modules || d.module_kind[d.xrow_mod[r]] != RMPC_MOD_ROWS) { err = "row description: xrow_mod must name a module of kind RMPC_MOD_ROWS"; return -1; }
  if (d.n_links < 0 || d.n_links > RMPC_MAX_LINKS || d.n_pairs < 0 || d.n_pairs > RMPC_MAX_PAIRS) { err = "links/pairs out of range"; return -1; }
  auto frame_ok = [&](int f) { return f >= 0 && f < d.n_joints; };
  if (!frame_ok(d.end_frame)) { err = "end_frame out of range"; return -1; }
  for (int j = 0; j < d.n_joints; j++) {
    M.joint_type[j] = d.joint_type[j];
    for (int c = 0; c < 3; c++) { M.joint_xyz[j][c] = d.joint_xyz[j][c]; M.joint_axis[j][c] = d.joint_axis[j][c]; }
    for (int c = 0; c < 9; c++) M.joint_rot[j][c] = d.joint_rot[j][c];
  }
  if (d.robot == RMPC_ROBOT_DIFFDRIVE) {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, o[3] = {0, 0, 0};
    for (int j = 0; j < d.n_joints; j++) {
      const double *t = d.joint_xyz[j];
      for (int r = 0; r < 3; r++) o[r] += R[3 * r] * t[0] + R[3 * r + 1] * t[1] + R[3 * r + 2] * t[2];
      double Rn[9];
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
          Rn[3 * r + c] = R[3 * r] * d.joint_rot[j][c] + R[3 * r + 1] * d.joint_rot[j][3 + c] + R[3 * r + 2] * d.joint_rot[j][6 + c];
      memcpy(R, Rn, sizeof R);
      for (int c = 0; c < 3; c++) M.dd_off[j][c] = o[c];
    }
  }
  M.off_r_body = d.off_r_body; M.off_obst = d.off_obst; M.off_lin = d.off_lin; M.off_wu = d.off_wu;
  M.off_goal = d.off_goal; M.off_wgoal = d.off_wgoal; M.off_wconstr = d.off_wconstr; M.off_ws = d.off_ws;
  M.has_goal = d.has_goal; M.has_avoid = d.has_avoid;
  auto off_ok = [&](int off, int len) { return off >= 0 && off + len <= d.npar; };
  if (!off_ok(d.off_wu, d.nu)) { err = "off_wu"; return -1; }
  if (d.ns && !off_ok(d.off_ws, 1)) { err = "off_ws"; return -1; }
  if (d.has_goal && (!off_ok(d.off_goal, 3) || !off_ok(d.off_wgoal, 3))) { err = "goal offsets"; return -1; }
  if (d.has_avoid && !off_ok(d.off_wconstr, d.n_modules)) { err = "off_wconstr"; return -1; }
  // general rows in module order
  int row = 0, nfk = 0;
  for (int mi = 0; mi < d.n_modules; mi++) {
    M.mod_kind[mi] = d.module_kind[mi];
    M.mod_row0[mi] = row;
    auto push = [&](int kind, int a, int bb, int poff, bool fk) -> bool {
      if (row >= kMaxRows) return false;
      M.row_kind[row] = (int8_t)kind; M.row_a[row] = (int8_t)a; M.row_b[row] = (int8_t)bb;
      M.row_poff[row] = poff; M.row_fk[row] = fk ? (int8_t)nfk++ : (int8_t)-1; M.row_mod[row] = (int8_t)mi;
      row++;
      return true;
    };
    bool ok = true;
    switch (d.module_kind[mi]) {
      case RMPC_MOD_RADIAL:
        if (!off_ok(d.off_r_body, 1) || !off_ok(d.off_obst, 4 * d.nobst)) { err = "radial offsets"; return -1; }
        for (int l = 0; l < d.n_links && ok; l++) {
          if (!frame_ok(d.link_frame[l])) { err = "link frame"; return -1; }
          for (int i = 0; i < d.nobst && ok; i++) ok = push(ROW_RADIAL, d.link_frame[l], i, 0, true);
        }
        break;
      case RMPC_MOD_LINEAR:
        if (!off_ok(d.off_r_body, 1) || !off_ok(d.off_lin, 4 * d.nobst)) { err = "linear offsets"; return -1; }
        for (int l = 0; l < d.n_links && ok; l++) {
          if (!frame_ok(d.link_frame[l])) { err = "link frame"; return -1; }
          for (int i = 0; i < d.nobst && ok; i++) ok = push(ROW_LINEAR, d.link_frame[l], i, 0, true);
        }
        break;
      case RMPC_MOD_SELFCOLLISION:
        if (d.n_pairs > 0 && !off_ok(d.off_r_body, 1)) { err = "self collision offsets"; return -1; }
        for (int pi = 0; pi < d.n_pairs && ok; pi++) {
          if (!frame_ok(d.pair_frame[pi][0]) || !frame_ok(d.pair_frame[pi][1])) { err = "pair frame"; return -1; }
          ok = push(ROW_SELF, d.pair_frame[pi][0], d.pair_frame[pi][1], 0, true);
        }
        break;
      case RMPC_MOD_JOINTLIMIT:
        if (!off_ok(d.off_lower, d.n) || !off_ok(d.off_upper, d.n)) { err = "joint limit offsets"; return -1; }
        for (int j = 0; j < d.n && ok; j++) {
          ok = push(ROW_SINGLE, j, +1, d.off_lower + j, false);
          ok = ok && push(ROW_SINGLE, j, -1, d.off_upper + j, false);
        }
        break;
      case RMPC_MOD_VELLIMIT:
        if (!off_ok(d.off_lower_vel, 2) || !off_ok(d.off_upper_vel, 2)) { err = "velocity limit offsets"; return -1; }
        for (int j = 0; j < 2 && ok; j++) {
          ok = push(ROW_SINGLE, d.nx - 2 + j, +1, d.off_lower_vel + j, false);
          ok = ok && push(ROW_SINGLE, d.nx - 2 + j, -1, d.off_upper_vel + j, false);
        }
        break;
      case RMPC_MOD_INPUTLIMIT:
        if (!off_ok(d.off_lower_u, d.nu) || !off_ok(d.off_upper_u, d.nu)) { err = "input limit offsets"; return -1; }
        for (int j = 0; j < d.nu && ok; j++) {
          ok = push(ROW_SINGLE, d.nx + d.ns + j, +1, d.off_lower_u + j, false);
          ok = ok && push(ROW_SINGLE, d.nx + d.ns + j, -1, d.off_upper_u + j, false);
        }
        break;
      case RMPC_MOD_ROWS: {
        // a module given as row descriptions (rmpc.h): variants of the six kinds through the same row tables
        int on_x = 0, on_u = 0;
        for (int r = 0; r < d.n_xrows && ok; r++) {
          if (d.xrow_mod[r] != mi) continue;
          const int a = d.xrow_a[r], b = d.xrow_b[r], po = d.xrow_poff[r];
          switch (d.xrow_kind[r]) {
            case RMPC_ROW_RADIAL:
            case RMPC_ROW_LINEAR: {
              const bool radial = d.xrow_kind[r] == RMPC_ROW_RADIAL;
              int &base = radial ? M.off_obst : M.off_lin;
              if (!frame_ok(a)) { err = "row description: frame"; return -1; }
              if (!off_ok(d.off_r_body, 1) || !off_ok(po, 4)) { err = "row description: parameter offsets"; return -1; }
              if (base < 0) base = po;   // (no module of the kind: the list starts at the first described row)
              if (po < base || (po - base) % 4 != 0 || (po - base) / 4 > 63) {
                err = "row description: a sphere / plane must lie a multiple of 4 (at most 252) parameters behind the obstacle / plane list";
                return -1;
              }
              ok = push(radial ? ROW_RADIAL : ROW_LINEAR, a, (po - base) / 4, 0, true);
              on_x++;
              break;
            }
            case RMPC_ROW_SELF:
              if (!frame_ok(a) || !frame_ok(b) || a == b) { err = "row description: pair frames"; return -1; }
              if (!off_ok(d.off_r_body, 1)) { err = "row description: r_body"; return -1; }
              ok = push(ROW_SELF, a, b, 0, true);
              on_x++;
              break;
            case RMPC_ROW_VAR:
              if (a < 0 || a >= M.nv || (d.ns && a == d.nx)) { err = "row description: variable"; return -1; }
              if (b != 1 && b != -1) { err = "row description: sign must be +1 or -1"; return -1; }
              if (!off_ok(po, 1)) { err = "row description: limit offset"; return -1; }
              ok = push(ROW_SINGLE, a, b, po, false);
              (a < d.nx ? on_x : on_u)++;
              break;
            default:
              err = "row description: unknown row kind";
              return -1;
          }
        }
        if (on_x && on_u) { err = "row description: the rows of a module must all be on states or all on inputs"; return -1; }
        break;
      }
      default:
        err = "unknown constraint module";
        return -1;
    }
    if (!ok) { err = "too many inequality rows"; return -1; }
    M.mod_rows[mi] = row - M.mod_row0[mi];
  }
  M.nh = row; M.nfk = nfk;
  for (int j = 0; j < M.nv; j++)
    if (std::isfinite(d.lb[j])) { M.lb_var[M.nlb] = (int8_t)j; M.lb_val[M.nlb] = d.lb[j]; M.nlb++; }
  for (int j = 0; j < M.nv; j++)
    if (std::isfinite(d.ub[j])) { M.ub_var[M.nub] = (int8_t)j; M.ub_val[M.nub] = d.ub[j]; M.nub++; }
  M.m = M.nh + M.nlb + M.nub;
  M.max_iter = d.max_iter > 0 ? d.max_iter : 200;
  M.tol_stat = d.tol_stat > 0 ? d.tol_stat : 1e-6;
  M.tol_eq = d.tol_eq > 0 ? d.tol_eq : 1e-8;
  M.tol_ineq = d.tol_ineq > 0 ? d.tol_ineq : 1e-8;
  M.tol_comp = d.tol_comp > 0 ? d.tol_comp : 1e-6;
  M.mu0 = d.mu0 > 0 ? d.mu0 : 1.0;
  M.acc_iters = d.acc_iters < 0 ? 0 : d.acc_iters;
  M.acc_obj_tol = d.acc_obj_tol > 0 ? d.acc_obj_tol : 1e-8;
  M.ls_max = d.ls_max > 0 ? d.ls_max : kLsMax;
  // exact curvature of the distance rows: holonomic chain, no slack, and for n <= 3 every frame a
  // distance row refers to moves affinely with q (prismatic joints, or revolute at the frame itself)
  auto affine = [&](int f) {
    for (int j = 0; j <= f; j++)
      if (d.joint_type[j] == RMPC_JOINT_REVOLUTE && j != f) return false;
    return true;
  };
  bool curv = d.robot == RMPC_ROBOT_CHAIN && d.ns == 0;
  // (the arms carry the kinematics' own second derivatives: Cfg::FKCURV)
  // (by row: the sphere and pair rows of the built-in modules and of the row-described ones alike)
  for (int r = 0; r < M.nh && curv && d.n <= 3; r++) {
    if (M.row_kind[r] == ROW_RADIAL) curv = curv && affine(M.row_a[r]);
    if (M.row_kind[r] == ROW_SELF) curv = curv && affine(M.row_a[r]) && affine(M.row_b[r]);
  }
  if (d.robot == RMPC_ROBOT_DIFFDRIVE) curv = true;   // exact second-order terms of the unicycle (Cfg::DDCURV)
  M.use_curv = curv ? 1 : 0;
  return 0;
}

// ---- generated views (rmpc_spec_gen.hpp) --------------------------------------------------
// Source text of the view of one descriptor: the accessors of RtView as constexpr functions over literal tables
// (doubles as hex floats: exact).  scripts/gen_specs.py writes rmpc_spec_gen.hpp from it for the shipped
// configurations; the library is then built with those views next to the runtime one.
static std::string spec_source(const rmpc_desc &d, const DevModel &M, const DevTables &T, const std::string &name) {
  std::string o;
  char buf[128];
  auto fi = [&](int v) { snprintf(buf, sizeof buf, "%d", v); return std::string(buf); };
  auto fd = [&](double v) { snprintf(buf, sizeof buf, "%a", v); return std::string(buf); };
  auto scalar = [&](const char *nm, int v) {
    o += "  __host__ __device__ static constexpr int " + std::string(nm) + "() { return " + fi(v) + "; }\n";
  };
  auto arr1 = [&](const char *nm, const int *p, int n) {
    o += "  __host__ __device__ static constexpr int " + std::string(nm) + "(int i) { constexpr int t[" + fi(n) + "] = {";
    for (int i = 0; i < n; i++) o += (i ? ", " : "") + fi(p[i]);
    o += "}; return t[i]; }\n";
  };
  auto arr2i = [&](const char *nm, const int *p, int n0, int n1) {
    o += "  __host__ __device__ static constexpr int " + std::string(nm) + "(int i, int j) { constexpr int t[" + fi(n0) + "][" + fi(n1) + "] = {";
    for (int i = 0; i < n0; i++) {
      o += (i ? ", {" : "{");
      for (int j = 0; j < n1; j++) o += (j ? ", " : "") + fi(p[i * n1 + j]);
      o += "}";
    }
    o += "}; return t[i][j]; }\n";
  };
  auto arr2d = [&](const char *nm, const double *p, int n0, int n1) {
    o += "  __host__ __device__ static constexpr double " + std::string(nm) + "(int i, int j) { constexpr double t[" + fi(n0) + "][" + fi(n1) + "] = {";
    for (int i = 0; i < n0; i++) {
      o += (i ? ", {" : "{");
      for (int j = 0; j < n1; j++) o += (j ? ", " : "") + fd(p[i * n1 + j]);
      o += "}";
    }
    o += "}; return t[i][j]; }\n";
  };
  o += "struct " + name + " {\n  static constexpr bool SPEC = true;\n";
  o += "  static constexpr int ROBOT = " + fi(d.robot) + ", NQ = " + fi(d.n) + ", NS = " + fi(d.ns) + ";\n";
  o += "  __host__ __device__ " + name + "() {}\n  __host__ __device__ " + name + "(const DevModel &, const DevTables &) {}\n";
  scalar("nslots", T.nslots);
  arr1("slot_fa", T.slot_fa, kMaxSlots);
  arr1("slot_fb", T.slot_fb, kMaxSlots);
  arr1("slot_row_begin", T.slot_row_begin, kMaxSlots + 1);
  scalar("nfkrows", T.nfkrows);
  arr1("fk_row", T.fk_row, kMaxFkRows);
  arr1("fk_kind", T.fk_kind, kMaxFkRows);
  arr1("fk_obst", T.fk_obst, kMaxFkRows);
  arr1("fk_mod", T.fk_mod, kMaxFkRows);
  arr1("fk_first", T.fk_first, kMaxFkRows);
  arr1("fk_idx", T.fk_idx, kMaxFkRows);
  arr2i("v_row", &T.v_row[0][0], RMPC_NV_MAX, kVarRows);
  arr2i("v_sgn", &T.v_sgn[0][0], RMPC_NV_MAX, kVarRows);
  arr2i("v_poff", &T.v_poff[0][0], RMPC_NV_MAX, kVarRows);
  arr2i("v_soft", &T.v_soft[0][0], RMPC_NV_MAX, kVarRows);
  arr2i("v_mod", &T.v_mod[0][0], RMPC_NV_MAX, kVarRows);
  arr2i("v_first", &T.v_first[0][0], RMPC_NV_MAX, kVarRows);
  arr2d("v_val", &T.v_val[0][0], RMPC_NV_MAX, kVarRows);
  scalar("off_r_body", M.off_r_body); scalar("off_obst", M.off_obst); scalar("off_lin", M.off_lin);
  scalar("off_wu", M.off_wu); scalar("off_goal", M.off_goal); scalar("off_wgoal", M.off_wgoal);
  scalar("off_wconstr", M.off_wconstr); scalar("off_ws", M.off_ws);
  scalar("has_goal", M.has_goal); scalar("has_avoid", M.has_avoid);
  arr1("joint_type", M.joint_type, RMPC_MAX_JOINTS);
  arr2d("joint_xyz", &M.joint_xyz[0][0], RMPC_MAX_JOINTS, 3);
  arr2d("joint_rot", &M.joint_rot[0][0], RMPC_MAX_JOINTS, 9);
  arr2d("joint_axis", &M.joint_axis[0][0], RMPC_MAX_JOINTS, 3);
  arr2d("dd_off", &M.dd_off[0][0], RMPC_MAX_JOINTS, 3);
  o += "};\n";
  return o;
}

// ---- workspace carving ---------------------------------------------------------------
struct Carver {
  char *base;
  size_t off = 0;
  explicit Carver(void *b) : base((char *)b) {}
  template <class T>
  T *take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T *p = base ? (T *)(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
};

// rs: stage-record stride (Cfg::RS)
static size_t carve(const DevModel &M, int rs, int Bp, int max_passes, void *base, Ws &W) {
  Carver c(base);
  const size_t S = (size_t)M.N * Bp;  // one slot
  const int nq = M.n, nq2 = nq * (nq + 1) / 2;
  W.N = M.N; W.Bp = Bp;
  W.p = c.take<double>(S * M.npar);
  for (int i = 0; i < 2; i++) {
    W.z[i] = c.take<double>(S * M.nv);
    W.t[i] = c.take<double>(S * M.m);
    W.lam[i] = c.take<double>(S * M.m);
    W.nu[i] = c.take<double>(S * M.nx);
  }
  W.dz = c.take<double>(S * M.nv);
  W.nunew = c.take<double>(S * M.nx);
  W.rs = rs;
  W.R = c.take<double>(S * W.rs);
  W.gfa = c.take<double>(S * M.nv);
  for (int i = 0; i < 2; i++) {
    W.grow[i] = c.take<double>(S * (M.nh > 0 ? M.nh : 1));
    W.Jq[i] = c.take<double>(S * (M.nfk > 0 ? M.nfk * nq : 1));
  }
  W.kps = (M.nw * M.nx + M.nw + M.nx * (M.nx + 1) / 2 + M.nx + M.nx + 8) / 8 * 8;   // (>= one spare word behind the image: stores of idle lanes)
  W.KP = c.take<double>(S * W.kps);
  W.part = c.take<double>(S * P_COUNT);
  W.gphi = c.take<double>(S);
  W.amin_p = c.take<unsigned long long>(Bp);
  W.amin_d = c.take<unsigned long long>(Bp);
  double **per[] = {&W.mu, &W.rho, &W.phi0, &W.Dd, &W.fcur, &W.thcur, &W.logcur,
                    &W.res_stat, &W.res_eq, &W.res_ineq, &W.res_comp, &W.obj, &W.mu_hold, &W.theta_mem, &W.theta_c};
  for (auto pp : per) *pp = c.take<double>(Bp);
  int **peri[] = {&W.status, &W.iters, &W.ls, &W.cur, &W.newstep, &W.redo, &W.force_gn, &W.gn_sticky, &W.curv_fail, &W.usedc, &W.stall,
                  &W.ls0, &W.lsst, &W.curv_skip, &W.curv_back, &W.small_steps, &W.theta_clean, &W.theta_retry};
  for (auto pp : peri) *pp = c.take<int>(Bp);
  W.active_hist = c.take<int>(max_passes + 8);
  W.act_idx = c.take<int>(Bp);
  W.n_act = c.take<int>(64);
  W.orig = c.take<int>(Bp);
  W.wlam = c.take<double>(S * M.m);
  W.wnu = c.take<double>(S * M.nx);
  W.wmu = c.take<double>(Bp);
  return (c.off + 255) & ~(size_t)255;
}

static int passes_cap(const DevModel &M) { return 4 * M.max_iter + 64; }
// columns of the compact workspace (0: batches of this handle never migrate)
static int compact_columns(int max_batch) {
  return max_batch >= kMigrateMin ? ((max_batch + kDenseDiv - 1) / kDenseDiv + 63) / 64 * 64 : 0;
}

// Algorithmic bytes (DESIGN.md, section "Kernels"): what one ACTIVE lane must read and
// write by design.  Sweep / step lanes are (instance, stage) pairs, riccati lanes are
// instances (bytes already multiplied by N stages).  pack / unpack are per call.
static void fill_lane_bytes(rmpc_handle *h, int B) {
  const DevModel &M = h->M;
  const int nq2 = M.n * (M.n + 1) / 2;
  const int64_t dd = (M.robot == RMPC_ROBOT_DIFFDRIVE) ? 35 : 0;
  const int64_t sweep_rd = M.nv * 2 + M.m * 2 + M.nfk * (1 + M.n) + M.nx * 4 + M.npar + M.nx * 2 + 2;
  // stage record (k_sweep -> k_riccati): Qqq, Cqq, Dg, cs, q0, q1, rc, A5 B5, zero slot
  const int64_t rec = 2 * nq2 + (M.nv - M.n) + (M.ns ? M.nv : 0) + 2 * M.nv + M.nx + dd + 1;
  const int64_t sweep_wr = M.nv + 2 * M.m + M.nx + rec + M.nv + M.nh + M.nfk * M.n + P_COUNT;
  // gain record (k_riccati backward -> forward): K, kff, P (packed), p, rc
  const int64_t kpw = M.nw * M.nx + M.nw + M.nx * (M.nx + 1) / 2 + 2 * M.nx;
  const int64_t ric_rd = P_COUNT + 3 + rec + kpw + dd;
  const int64_t ric_wr = kpw + M.nv + M.nx;
  const int64_t step_rd = 3 * M.nv + 2 * M.m + M.nh + M.nfk * M.n;
  const int64_t step_wr = 3;  // gphi and two atomic minima (the row steps are recomputed by k_sweep, not stored)
  h->lane_bytes[K_PACK] = 16 * ((int64_t)B * (M.nx + (int64_t)M.N * (M.nv + M.npar)));
  h->lane_bytes[K_SWEEP] = 8 * (sweep_rd + sweep_wr);
  h->lane_bytes[K_RICCATI] = 8 * (int64_t)M.N * (ric_rd + ric_wr);
  h->lane_bytes[K_STEP] = 8 * (step_rd + step_wr);
  h->lane_bytes[K_UNPACK] = 16 * (int64_t)B * M.N * M.nv;
  // fused kernel, per instance: the compulsory I/O of a solve: xinit, x0, parameters in, plan and
  // four statistics out -- everything in between is the owner wavefront's private state
  h->lane_bytes[K_FUSED] = 8 * ((int64_t)M.nx + 2 * (int64_t)M.N * M.nv + (int64_t)M.N * M.npar) + 24;
}

static hipEvent_t prof_event(rmpc_handle *h) {
  if (h->ev_used == h->ev.size()) {
    hipEvent_t e;
    (void)hipEventCreate(&e);
    h->ev.push_back(e);
  }
  return h->ev[h->ev_used++];
}

struct ProfScope {
  rmpc_handle *h;
  hipStream_t st;
  int kind;
  ProfScope(rmpc_handle *h_, hipStream_t st_, int kind_) : h(h_), st(st_), kind(kind_) {
    if (h->profiling) (void)hipEventRecord(prof_event(h), st);
  }
  ~ProfScope() {
    if (h->profiling) {
      (void)hipEventRecord(prof_event(h), st);
      h->ev_kind.push_back(kind);
    }
  }
};

static void prof_collect(rmpc_handle *h) {
  for (size_t i = 0; i < h->ev_kind.size(); i++) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, h->ev[2 * i], h->ev[2 * i + 1]);
    h->prof_ms[h->ev_kind[i]] += ms;
    h->prof_n[h->ev_kind[i]]++;
  }
  h->ev_used = 0;
  h->ev_kind.clear();
}

// ---- fused path ------------------------------------------------------------------------------------------
static int fused_columns(int max_batch) { return (max_batch + 1) / 2 * 2; }
static size_t carve_fused(const DevModel &M, const VariantOps &v, int Bcap, void *base, FusedWs &F) {
  Carver c(base);
  const size_t S = (size_t)Bcap * kFusedStages;
  const bool arm = v.arm_fused;
  F.nv = M.nv; F.m = M.m; F.nx = M.nx; F.npar = M.npar;
  // (the arms: one spare row behind the general rows' values, where the rows that keep no value are stored)
  F.nhs = arm ? M.nh + 1 : (M.nh > 0 ? M.nh : 1); F.njqs = M.nfk > 0 ? M.nfk * M.n : 1;
  F.p = c.take<double>(S * M.npar);
  // (the arms: F.m counts the spare row behind the slacks / multipliers, where the rows a joint does not have are evaluated)
  if (arm) F.m = M.m + 1;
  for (int i = 0; i < 2; i++) {
    F.z[i] = c.take<double>(S * M.nv);
    F.t[i] = c.take<double>(S * F.m);
    F.lam[i] = c.take<double>(S * F.m);
    F.nu[i] = c.take<double>(S * M.nx);
    F.grow[i] = c.take<double>(S * F.nhs);
    F.Jq[i] = c.take<double>(S * F.njqs);
  }
  F.dz = c.take<double>(S * M.nv);
  F.nunew = c.take<double>(S * M.nx);
  F.gfa = c.take<double>(S * M.nv);
  F.wlam = c.take<double>(S * F.m);
  F.wnu = c.take<double>(S * M.nx);
  F.wmu = c.take<double>(Bcap);
  F.rs = v.rs;
  // (the arms: a record slot for every one of the 32 stage columns -- lanes without a stage work on the padding columns)
  F.R = c.take<double>((size_t)Bcap * (arm ? kFusedStages : M.N) * F.rs);
  F.kps = (M.nw * M.nx + M.nw + M.nx * (M.nx + 1) / 2 + M.nx + M.nx + 8) / 8 * 8;
  F.KP = c.take<double>((size_t)Bcap * M.N * F.kps);
  F.passes = c.take<int>(64);
  F.lastp = c.take<int>(Bcap);
  F.order = c.take<int>(Bcap);
  F.ckey = c.take<int>(Bcap);
  F.stamps = c.take<long long>((size_t)Bcap * 8);
  return (c.off + 255) & ~(size_t)255;
}
// k_fused_arm reads the row STRUCTURE of a joint's variables (which limit / bound rows q_a, v_a, u_a have, whether a
// row's limit is a parameter, its sign) from joint 0 and takes scalar branches on it; only row index, parameter offset
// and module differ from joint to joint.  True for every module of the reference (they loop over all joints:
// JointLimitConstraints.py:8-31, InputLimitConstraints.py:7-29, bounds mpcModel.py:91-104); checked here all the same.
static bool arm_rows_uniform(const DevModel &M, const DevTables &T) {
  const int keep = (1 << 8) | (1 << 9) | (1 << 11);
  for (int a = 1; a < M.n; a++)
    for (int c = 0; c < 3; c++)
      for (int u = 0; u < kVarRows; u++)
        if ((T.v_desc[a + c * M.n][u] & keep) != (T.v_desc[c * M.n][u] & keep)) return false;
  return true;
}
static bool fused_supported(const VariantOps *v, const DevModel &M, const DevTables &T) {
  // chain n = 3 and the diff-drive base, horizons that fit the 32 lanes of an instance.  The arm stays with the pass
  // kernels: in the fused kernel (measured twice in round 2, the second time with the recursion as a real function) a
  // pass takes 670 k cycles -- its recursion on the 32 lanes of an instance alone 347 k, twice the 64-lane pass kernel
  // -- against ~480 k for the four pass kernels.  Restructuring the arm's recursion like the chain's (records straight
  // into registers, three ordering points per stage) changed nothing either (6.8 vs 7.0 ms per batch): it is bound by
  // the 7 x 7 factorisation and the cost-to-go update, not by its ordering points.
  return v && v->fused && (!v->arm_fused || arm_rows_uniform(M, T)) && M.N <= kFusedStages;
}

static void launch_fused(rmpc_handle *h, int B, const double *d_xinit, const double *d_x0, const double *d_params,
                         double *d_zout, int *d_exit, int *d_iters, double *d_kkt, double *d_obj, hipStream_t st, int cap) {
  const VariantOps &v = *h->ops;
  const int warm = (h->warm_mode && h->have_duals) ? 1 : 0;
  // closed loop: the previous solve of this batch tells which instances take long (k_fused: launch order)
  int use_order = (warm && !h->env_no_order) ? 1 : 0;
  // cold launch with a queue behind the grid (more instance pairs than wavefronts): the instances closest to a
  // constraint boundary first (k_difficulty)
  // (holonomic chains only: measured on the BASELINE batches, one launch alone 3.05 -> 2.59 ms for the point robots,
  //  14.7 -> 15.0 ms for the boxers, whose slow instances are slow for another reason -- the Gauss-Newton blocks of the
  //  unicycle converge linearly -- and gain nothing from the two little kernels in front of the launch)
  if (v.difficulty && v.robot == RMPC_ROBOT_CHAIN && !warm && !h->env_no_order && !h->env_no_cold_order && d_params &&
      (B + 1) / 2 > h->fused_grid) {
    v.difficulty(h, B, d_xinit, d_params, st);
    hipLaunchKernelGGL(k_order_t<64>, dim3(1), dim3(64), 0, st, (const int *)h->F.ckey, h->F.order, B);
    use_order = 1;
  }
  v.fused_launch(h, B, d_xinit, d_x0, d_params, d_zout, d_exit, d_iters, d_kkt, d_obj, st, cap, warm, use_order);
  // the order of the NEXT warm-started launch, right behind this one (in front of it the little kernel would wait
  // for a free SIMD whenever another handle's fused launch fills the chip: 130 us in the fleet loop)
  if (h->warm_mode && !h->env_no_order)
    hipLaunchKernelGGL(k_order_t<1024>, dim3(1), dim3(1024), 0, st, (const int *)h->F.lastp, h->F.order, B);
}

static int solve_device(rmpc_handle *h, int B, const double *d_xinit, const double *d_x0, const double *d_params,
                        double *d_zout, int *d_exit, int *d_iters, double *d_kkt, double *d_obj, hipStream_t st,
                        int max_passes_override) {
  if (B < 1 || B > h->max_batch) return fail("batch size out of range for this handle");
  const DevModel &M = h->M;
  HIPCHK(hipSetDevice(h->device));
  fill_lane_bytes(h, B);
  if (h->have_duals && h->duals_B != B) h->have_duals = false;   // multipliers of another batch: cold start
  if (d_params) h->packed_B = 0;   // (the workspace parameters are about to be overwritten)
  if (h->fused) {
    // one launch: every wavefront carries its two instances from the first sweep to the plan
    int cap = max_passes_override > 0 ? max_passes_override : h->max_passes;
    if (h->pass_budget > 0 && h->pass_budget < cap) cap = h->pass_budget;
    HIPCHK(hipMemsetAsync(h->F.passes, 0, 16, st));   // [0] most passes of an instance, [1] queue counter
    {
      ProfScope ps(h, st, K_FUSED);
      launch_fused(h, B, d_xinit, d_x0, d_params, d_zout, d_exit, d_iters, d_kkt, d_obj, st, cap);
    }
    HIPCHK(hipGetLastError());
    h->have_duals = true; h->duals_B = B;   // (the kernel has left the multipliers in the warm-start arrays)
    h->last_passes = -1;   // on the device (rmpc_last_passes fetches it)
    if (h->profiling) {
      HIPCHK(hipStreamSynchronize(st));
      prof_collect(h);
      h->prof_bytes[K_FUSED] += (double)B * (double)h->lane_bytes[K_FUSED];
    }
    return 0;
  }
  HIPCHK(hipMemsetAsync(h->W.active_hist, 0, sizeof(int) * (h->max_passes + 8), st));
  {
    ProfScope ps(h, st, K_PACK);
    dim3 g1((B + 63) / 64, (M.N * M.npar + 63) / 64);
    if (d_params)  // nullptr: the parameters were written straight into W.p by rmpc_solve_batch_scene_device
      hipLaunchKernelGGL(k_pack, g1, dim3(256), 0, st, d_params, h->W.p, B, M.N * M.npar, M.npar, M.N, h->Bp);
    dim3 g2((B + 63) / 64, (M.N * M.nv + 63) / 64);
    hipLaunchKernelGGL(k_pack, g2, dim3(256), 0, st, d_x0, h->W.z[0], B, M.N * M.nv, M.nv, M.N, h->Bp);
    hipLaunchKernelGGL(k_init, dim3((B + 255) / 256), dim3(256), 0, st, h->W, d_xinit, B, M.nx, M.mu0,
                       (h->warm_mode && h->have_duals) ? 1 : 0);
  }
  int cap = max_passes_override > 0 ? max_passes_override : h->max_passes;
  if (h->pass_budget > 0 && h->pass_budget < cap) cap = h->pass_budget;
  int pass = 0, next_check = 8;
  Phase ph{h->W, B};
  bool migrated = false;
  const bool may_migrate = h->Bpc > 0 && B >= kMigrateMin && !h->env_no_migrate;
  // A solve with a deadline in passes (rmpc_set_pass_budget) is enqueued whole, without a host look: every kernel
  // leaves at once when the list of iterating instances is empty, so the call returns immediately and the solve is
  // ordered with the caller's stream like a fused launch (rmpc_is_async).  Without a deadline the host reads one
  // counter every few passes (it cannot know how many passes to enqueue) and moves the survivors to the compact
  // workspace.
  const bool async = h->pass_budget > 0 && max_passes_override <= 0;
  for (; pass < cap; pass++) {
    const int first = pass == 0;
    { ProfScope ps(h, st, K_SWEEP); h->ops->pass(h, ph, first, pass, st, K_SWEEP); }
    { ProfScope ps(h, st, K_RICCATI); h->ops->pass(h, ph, first, pass, st, K_RICCATI); }
    if (ph.B <= kCompactWaveMax) hipLaunchKernelGGL(k_compact_wave, dim3(1), dim3(64), 0, st, ph.W, ph.B, pass);
    else hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, st, ph.W, ph.B, pass);
    { ProfScope ps(h, st, K_STEP); h->ops->pass(h, ph, first, pass, st, K_STEP); }
    if (h->profiling) HIPCHK(hipGetLastError());   // per pass when profiling is on (otherwise once after the loop)
    if (!async && pass + 1 == next_check && max_passes_override <= 0) {
      HIPCHK(hipMemcpyAsync(h->h_active, h->W.active_hist + pass, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      const int n = *h->h_active;
      if (n == 0) { pass++; break; }
      if (may_migrate && !migrated && n * kDenseDiv <= B) {
        // k_compact has just left the compacted list of the n survivors in the batch's workspace
        hipLaunchKernelGGL(k_migrate, dim3((n + 63) / 64, M.N), dim3(64), 0, st, h->W, h->Wc, n, M.nv, M.m, M.nx, M.npar,
                           M.nh, M.nfk * M.n);
        ph = Phase{h->Wc, n};
        migrated = true;
      }
      next_check += (may_migrate && !migrated) ? 2 : 4;  // look more often while the migration is still ahead
    }
  }
  h->last_passes = async ? -2 : pass;   // (-2: on the device, rmpc_last_passes counts the non-empty passes of active_hist)
  h->last_cap = pass;
  {
    ProfScope ps(h, st, K_UNPACK);
    dim3 g((B + 63) / 64, (M.N * M.nv + 63) / 64);
    hipLaunchKernelGGL(k_unpack, g, dim3(256), 0, st, h->W, d_zout, d_exit, d_iters, d_kkt, d_obj, B, M.nv, (const int *)nullptr);
    if (migrated) {
      // the survivors' results overwrite the stale rows the first launch wrote for them
      dim3 gc((ph.B + 63) / 64, (M.N * M.nv + 63) / 64);
      hipLaunchKernelGGL(k_unpack, gc, dim3(256), 0, st, h->Wc, d_zout, d_exit, d_iters, d_kkt, d_obj, ph.B, M.nv,
                         (const int *)h->Wc.orig);
    }
  }
  if (h->warm_mode) {
    // multipliers for the next solve (the survivors' from the compact workspace, over the stale ones of the first launch)
    const int lanes = h->W.Bp * M.N;
    hipLaunchKernelGGL(k_save_duals, dim3((lanes + 255) / 256), dim3(256), 0, st, h->W, h->W, B, M.m, M.nx, (const int *)nullptr, M.mu0);
    if (migrated) {
      const int lc = h->Wc.Bp * M.N;
      hipLaunchKernelGGL(k_save_duals, dim3((lc + 255) / 256), dim3(256), 0, st, h->Wc, h->W, ph.B, M.m, M.nx, (const int *)h->Wc.orig, M.mu0);
    }
    h->have_duals = true; h->duals_B = B;
  } else {
    h->have_duals = false;
  }
  HIPCHK(hipGetLastError());
  if (h->profiling) {
    // active (instance) lanes per pass: the sweep of pass p works on what was still
    // active after pass p-1, riccati likewise; step on what riccati p left active.
    h->h_hist.resize(pass + 1);
    HIPCHK(hipMemcpyAsync(h->h_hist.data(), h->W.active_hist, sizeof(int) * pass, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    prof_collect(h);
    double act_in = 0, act_out = 0;
    for (int p = 0; p < pass; p++) {
      act_in += (p == 0) ? B : h->h_hist[p - 1];
      act_out += h->h_hist[p];
    }
    h->prof_bytes[K_PACK] += (double)h->lane_bytes[K_PACK];
    h->prof_bytes[K_UNPACK] += (double)h->lane_bytes[K_UNPACK];
    h->prof_bytes[K_SWEEP] += act_in * M.N * (double)h->lane_bytes[K_SWEEP];
    h->prof_bytes[K_RICCATI] += act_in * (double)h->lane_bytes[K_RICCATI];
    h->prof_bytes[K_STEP] += act_out * M.N * (double)h->lane_bytes[K_STEP];
  }
  return 0;
}

#if defined(RMPC_STAMPS) || defined(RMPC_RIC_STAMPS)
// development aid: reads and clears the stamp counters of every variant unit (each code object holds its own copy;
// the entries of one unit share its reader) and returns their sums
static int sum_stamps(int (*VariantOps::*reader)(long long *), long long *out) {
  std::vector<int (*)(long long *)> seen;
  for (int i = 0; i < 8; i++) out[i] = 0;
  for (const VariantOps &v : variant_table()) {
    int (*const r)(long long *) = v.*reader;
    bool dup = false;
    for (auto q : seen) dup = dup || q == r;
    if (dup) continue;
    seen.push_back(r);
    long long part[8];
    if (r(part)) return 1;
    for (int i = 0; i < 8; i++) out[i] += part[i];
  }
  return 0;
}
#endif

extern "C" {

int rmpc_version(void) { return RMPC_VERSION; }
#ifndef RMPC_SOURCE_HASH
#define RMPC_SOURCE_HASH "unhashed"
#endif
const char *rmpc_source_hash(void) { return RMPC_SOURCE_HASH; }
const char *rmpc_last_error(void) { return g_err.c_str(); }
/* a descriptor of this version, or of 0.2.0 (the struct without the xrow_* arrays at its end: no row-described modules) */
static bool take_desc(const rmpc_desc *in, rmpc_desc &full) {
  if (!in) return false;
  const int old_size = (int)offsetof(rmpc_desc, n_xrows);
  if (in->struct_size != (int)sizeof(rmpc_desc) && in->struct_size != old_size) return false;
  memset(&full, 0, sizeof full);
  memcpy(&full, in, (size_t)in->struct_size);
  full.struct_size = (int)sizeof(rmpc_desc);
  return true;
}
/* generated views: source text for one descriptor, and which view a handle runs (see rmpc.h) */
int64_t rmpc_spec_source(const rmpc_desc *desc_in, const char *name, char *out, int64_t cap) {
  rmpc_desc dfull;
  if (!name || !take_desc(desc_in, dfull)) return fail("rmpc_spec_source: bad arguments");
  const rmpc_desc *desc = &dfull;
  DevModel M;
  DevTables T;
  std::string err;
  if (build_model(*desc, M, err) != 0 || build_tables(*desc, M, T, err) != 0) return fail("invalid descriptor: " + err);
  const std::string src = spec_source(*desc, M, T, name);
  if (out && cap > (int64_t)src.size()) memcpy(out, src.c_str(), src.size() + 1);
  return (int64_t)src.size() + 1;
}
const char *rmpc_spec_name(rmpc_handle *h) { return h ? h->ops->spec : ""; }
const char *rmpc_spec_for(const rmpc_desc *desc_in) {
  rmpc_desc dfull;
  if (!take_desc(desc_in, dfull)) return "";
  const rmpc_desc *desc = &dfull;
  DevModel M;
  DevTables T;
  std::string err;
  if (build_model(*desc, M, err) != 0 || build_tables(*desc, M, T, err) != 0) return "";
  const VariantOps *v = find_spec(*desc, M, T);
  return v ? v->spec : "";
}
int rmpc_desc_size(void) { return (int)sizeof(rmpc_desc); }
const char *rmpc_kernel_name(int idx) { return (idx >= 0 && idx < RMPC_NUM_KERNELS) ? kKernelNames[idx] : ""; }

int64_t rmpc_workspace_bytes(const rmpc_desc *desc_in, int max_batch) {
  rmpc_desc dfull;
  if (!take_desc(desc_in, dfull) || max_batch < 1) return -1;
  const rmpc_desc *desc = &dfull;
  DevModel M;
  std::string err;
  if (build_model(*desc, M, err) != 0) { g_err = err; return -1; }
  DevTables T;
  if (build_tables(*desc, M, T, err) != 0) { g_err = err; return -1; }
  Ws W;
  const int Bp = (max_batch + 63) / 64 * 64;
  const int Bpc = compact_columns(max_batch);
  FusedWs F;
  const VariantOps *v = variant_of(*desc);
  const int rs = v ? v->rs : rec_layout(M).rs;
  const size_t fused = fused_supported(v, M, T) ? carve_fused(M, *v, fused_columns(max_batch), nullptr, F) : 0;
  return (int64_t)(carve(M, rs, Bp, passes_cap(M), nullptr, W) + (Bpc ? carve(M, rs, Bpc, 0, nullptr, W) : 0) + fused);
}

int rmpc_create(const rmpc_desc *desc_in, int max_batch, rmpc_handle **out) {
  if (!desc_in || !out) return fail("null argument");
  rmpc_desc dfull;
  if (!take_desc(desc_in, dfull)) return fail("rmpc_desc size mismatch (ABI version?)");
  const rmpc_desc *desc = &dfull;
  if (max_batch < 1) return fail("max_batch must be >= 1");
  rmpc_handle *h = new rmpc_handle();
  h->desc = *desc;
  std::string err;
  if (build_model(*desc, h->M, err) != 0) { delete h; return fail("invalid descriptor: " + err); }
  if (build_tables(*desc, h->M, h->T, err) != 0) { delete h; return fail("invalid descriptor: " + err); }
  h->ops = variant_of(*desc);
  if (!h->ops) { delete h; return fail("no kernel variant for this robot (built: " + variant_list() + ")"); }
  // Generated views (rmpc_spec_gen.hpp: the point-robot configurations).  Measured in round 2: with the chip full the
  // throughput is the same as with the runtime tables (1.60-1.65 M solves/s either way: the fused kernel is bound by
  // the traffic of the iterate, not by its instruction count), one batch alone is 6 % faster (4.42 vs 4.69 ms: the
  // requests of the sweep leave ahead of the arithmetic).  RMPC_NO_SPEC=1 (read here once) forces the runtime tables.
  if (const VariantOps *spec = getenv("RMPC_NO_SPEC") ? nullptr : find_spec(*desc, h->M, h->T)) h->ops = spec;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { delete h; return fail("no HIP device available"); }
  if (desc->device < 0 || desc->device >= ndev) { delete h; return fail("device ordinal out of range"); }
  h->device = desc->device;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cus > 0) h->fused_grid = 4 * cus;
    if (const char *g = getenv("RMPC_FUSED_GRID")) { const int v = atoi(g); if (v > 0) h->fused_grid = v; }   // (development switch)
  }
  h->max_batch = max_batch;
  h->Bp = (max_batch + 63) / 64 * 64;
  h->max_passes = passes_cap(h->M);
  hipError_t e = hipSetDevice(h->device);
  if (e != hipSuccess) { delete h; return fail(std::string("hipSetDevice: ") + hipGetErrorString(e)); }
  Ws tmp;
  h->Bpc = compact_columns(max_batch);
  const int rs = h->ops->rs;
  const size_t big = carve(h->M, rs, h->Bp, h->max_passes, nullptr, tmp);
  const size_t small = h->Bpc ? carve(h->M, rs, h->Bpc, 0, nullptr, tmp) : 0;
  h->fused = fused_supported(h->ops, h->M, h->T) && !getenv("RMPC_NO_FUSED");   // (debugging switch: pass kernels only)
  FusedWs ftmp;
  h->ws_bytes = big + small + (h->fused ? carve_fused(h->M, *h->ops, fused_columns(max_batch), nullptr, ftmp) : 0);
  e = hipMalloc(&h->ws_base, h->ws_bytes);
  if (e != hipSuccess) { delete h; return fail(std::string("hipMalloc workspace: ") + hipGetErrorString(e)); }
  e = hipMemset(h->ws_base, 0, h->ws_bytes);
  // (the fill runs on the null stream and may still be in flight when hipMemset returns; solves run on
  //  non-blocking streams that do not wait for it)
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { (void)hipFree(h->ws_base); delete h; return fail(std::string("hipMemset workspace: ") + hipGetErrorString(e)); }
  carve(h->M, rs, h->Bp, h->max_passes, h->ws_base, h->W);
  if (h->Bpc) {
    carve(h->M, rs, h->Bpc, 0, (char *)h->ws_base + big, h->Wc);
    h->Wc.active_hist = h->W.active_hist;  // one history per batch, whichever workspace the pass ran in
  }
  if (h->fused) carve_fused(h->M, *h->ops, fused_columns(max_batch), (char *)h->ws_base + big + small, h->F);
  // (the row tables, and behind them a copy of the fused workspace's pointer block: the phase functions of the
  //  fused kernel take the instance's bases from there instead of receiving two dozen pointers per call)
  // behind the row tables: the fused workspace block and a copy of the model (ArmBlock: the phase functions of the fused
  // kernels read both through uniform pointers)
  e = hipMalloc((void **)&h->d_T, sizeof(DevTables) + sizeof(ArmBlock));
  if (e == hipSuccess) e = hipMemcpy(h->d_T, &h->T, sizeof(DevTables), hipMemcpyHostToDevice);
  if (e == hipSuccess && h->fused) e = hipMemcpy((void *)(h->d_T + 1), &h->F, sizeof(FusedWs), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy((char *)(h->d_T + 1) + offsetof(ArmBlock, M), &h->M, sizeof(DevModel), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(h->ws_base); delete h; return fail(std::string("row tables: ") + hipGetErrorString(e)); }
  e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipHostMalloc((void **)&h->h_active, sizeof(int), hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc((void **)&h->h_passes, sizeof(int), hipHostMallocDefault);
  if (e != hipSuccess) { rmpc_destroy(h); return fail(std::string("stream / pinned word: ") + hipGetErrorString(e)); }
  if (const char *rl = getenv("RMPC_RIC_LANE")) h->ric_lane = atoi(rl);   // (development switch)
  h->env_no_migrate = getenv("RMPC_NO_MIGRATE") != nullptr;
  h->env_arm_two_parts = getenv("RMPC_ARM_TWO_PARTS") != nullptr;   // (development switch: k_fused_arm with two parts per stage at every horizon)
  h->env_no_order = getenv("RMPC_NO_ORDER") != nullptr;   // (development switch: fused launches in index order)
  h->env_no_cold_order = getenv("RMPC_NO_COLD_ORDER") != nullptr;   // (development switch: cold fused launches in index order)
  *out = h;
  return 0;
}

void rmpc_destroy(rmpc_handle *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();   // a solve enqueued on a caller's stream may still be reading the workspace
  void *bufs[] = {h->ws_base, (void *)h->d_T, h->d_xinit, h->d_x0, h->d_params, h->d_zout, h->d_kkt, h->d_obj, h->d_exit, h->d_iters};
  for (void *p : bufs) (void)hipFree(p);
  for (auto e : h->ev) (void)hipEventDestroy(e);
  if (h->h_active) (void)hipHostFree(h->h_active);
  if (h->h_passes) (void)hipHostFree(h->h_passes);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

static int ensure_staging(rmpc_handle *h) {
  if (h->d_xinit) return 0;
  const DevModel &M = h->M;
  const size_t B = h->max_batch;
  HIPCHK(hipMalloc((void **)&h->d_xinit, sizeof(double) * B * M.nx));
  HIPCHK(hipMalloc((void **)&h->d_x0, sizeof(double) * B * M.N * M.nv));
  HIPCHK(hipMalloc((void **)&h->d_params, sizeof(double) * B * M.N * M.npar));
  HIPCHK(hipMalloc((void **)&h->d_zout, sizeof(double) * B * M.N * M.nv));
  HIPCHK(hipMalloc((void **)&h->d_kkt, sizeof(double) * B));
  HIPCHK(hipMalloc((void **)&h->d_obj, sizeof(double) * B));
  HIPCHK(hipMalloc((void **)&h->d_exit, sizeof(int) * B));
  HIPCHK(hipMalloc((void **)&h->d_iters, sizeof(int) * B));
  return 0;
}

int rmpc_solve_batch(rmpc_handle *h, int B, const double *xinit, const double *x0, const double *params,
                     double *z_out, int32_t *exitflag, int32_t *iters, double *kkt_res, double *obj) {
  if (!h || !xinit || !x0 || !params || !z_out || !exitflag) return fail("null argument");
  if (B < 1 || B > h->max_batch) return fail("batch size out of range for this handle");
  HIPCHK(hipSetDevice(h->device));
  if (ensure_staging(h) != 0) return -1;
  const DevModel &M = h->M;
  hipStream_t st = h->stream;
  HIPCHK(hipMemcpyAsync(h->d_xinit, xinit, sizeof(double) * B * M.nx, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(h->d_x0, x0, sizeof(double) * (size_t)B * M.N * M.nv, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(h->d_params, params, sizeof(double) * (size_t)B * M.N * M.npar, hipMemcpyHostToDevice, st));
  if (solve_device(h, B, h->d_xinit, h->d_x0, h->d_params, h->d_zout, h->d_exit, h->d_iters, h->d_kkt, h->d_obj, st, 0) != 0)
    return -1;
  HIPCHK(hipMemcpyAsync(z_out, h->d_zout, sizeof(double) * (size_t)B * M.N * M.nv, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(exitflag, h->d_exit, sizeof(int) * B, hipMemcpyDeviceToHost, st));
  if (iters) HIPCHK(hipMemcpyAsync(iters, h->d_iters, sizeof(int) * B, hipMemcpyDeviceToHost, st));
  if (kkt_res) HIPCHK(hipMemcpyAsync(kkt_res, h->d_kkt, sizeof(double) * B, hipMemcpyDeviceToHost, st));
  if (obj) HIPCHK(hipMemcpyAsync(obj, h->d_obj, sizeof(double) * B, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

int rmpc_solve_batch_device(rmpc_handle *h, int B, const double *d_xinit, const double *d_x0, const double *d_params,
                            double *d_z_out, int32_t *d_exitflag, int32_t *d_iters, double *d_kkt_res,
                            double *d_obj, void *stream) {
  if (!h || !d_xinit || !d_x0 || !d_params || !d_z_out || !d_exitflag || !d_iters || !d_kkt_res || !d_obj)
    return fail("null argument");
  hipStream_t st = (hipStream_t)stream;   // NULL: the legacy null stream, ordered with the caller's default-stream work
  return solve_device(h, B, d_xinit, d_x0, d_params, d_z_out, d_exitflag, d_iters, d_kkt_res, d_obj, st, 0);
}

static void scene_args(const rmpc_handle *h, const rmpc_scene *s, SceneDev &S, SceneOff &O) {
  const rmpc_desc &d = h->desc;
  S.goal = s->goal; S.r_body = s->r_body; S.obst = s->obst; S.obst_dyn = s->obst_dyn;
  S.lower = s->lower_limits; S.upper = s->upper_limits; S.lower_u = s->lower_limits_u; S.upper_u = s->upper_limits_u;
  S.lower_vel = s->lower_limits_vel; S.upper_vel = s->upper_limits_vel; S.lin = s->lin_constrs;
  S.dyn_radius = s->dyn_radius; S.w = s->w; S.wu = s->wu; S.ws = s->ws;
  for (int i = 0; i < RMPC_MAX_MODULES; i++) S.wconstr[i] = s->wconstr[i];
  O.r_body = d.off_r_body; O.obst = d.off_obst; O.lin = d.off_lin; O.lower = d.off_lower; O.upper = d.off_upper;
  O.lower_u = d.off_lower_u; O.upper_u = d.off_upper_u; O.lower_vel = d.off_lower_vel; O.upper_vel = d.off_upper_vel;
  O.wu = d.off_wu; O.goal = d.has_goal ? d.off_goal : -1; O.wgoal = d.has_goal ? d.off_wgoal : -1;
  O.wconstr = d.has_avoid ? d.off_wconstr : -1; O.ws = d.ns ? d.off_ws : -1;
  O.n = d.n; O.nu = d.nu; O.nobst = d.nobst; O.n_modules = d.n_modules; O.npar = d.npar; O.N = d.N; O.dt = d.dt;
}

int rmpc_pack_scene_device(rmpc_handle *h, int B, const rmpc_scene *scene, double *d_params, void *stream) {
  if (!h || !scene || !d_params) return fail("null argument");
  if (scene->struct_size != (int)sizeof(rmpc_scene)) return fail("rmpc_scene size mismatch");
  if (B < 1 || B > h->max_batch) return fail("batch size out of range for this handle");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;   // NULL: the legacy null stream, ordered with the caller's default-stream work
  SceneDev S; SceneOff O;
  scene_args(h, scene, S, O);
  const int lanes = B * h->M.N;
  hipLaunchKernelGGL((k_scene<0>), dim3((lanes + 255) / 256), dim3(256), 0, st, S, O, d_params, B, h->Bp);
  HIPCHK(hipGetLastError());
  return 0;
}

int rmpc_pack_scene_workspace(rmpc_handle *h, int B, const rmpc_scene *scene, void *stream) {
  if (!h || !scene) return fail("null argument");
  if (scene->struct_size != (int)sizeof(rmpc_scene)) return fail("rmpc_scene size mismatch");
  if (B < 1 || B > h->max_batch) return fail("batch size out of range for this handle");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;   // NULL: the legacy null stream, ordered with the caller's default-stream work
  SceneDev S; SceneOff O;
  scene_args(h, scene, S, O);
  if (h->fused) {
    const int lanes = B * h->M.N;
    hipLaunchKernelGGL((k_scene<2>), dim3((lanes + 255) / 256), dim3(256), 0, st, S, O, h->F.p, B, h->Bp);
  } else {
    const int lanes = h->Bp * h->M.N;
    hipLaunchKernelGGL((k_scene<1>), dim3((lanes + 255) / 256), dim3(256), 0, st, S, O, h->W.p, B, h->Bp);
  }
  HIPCHK(hipGetLastError());
  h->packed_B = B;
  return 0;
}

int rmpc_solve_batch_packed_device(rmpc_handle *h, int B, const double *d_xinit, const double *d_x0, double *d_z_out,
                                   int32_t *d_exitflag, int32_t *d_iters, double *d_kkt_res, double *d_obj, void *stream) {
  if (!h || !d_xinit || !d_x0 || !d_z_out || !d_exitflag || !d_iters || !d_kkt_res || !d_obj) return fail("null argument");
  if (h->packed_B != B) return fail("no parameters of this batch size in the workspace (rmpc_pack_scene_workspace first)");
  return solve_device(h, B, d_xinit, d_x0, nullptr, d_z_out, d_exitflag, d_iters, d_kkt_res, d_obj, (hipStream_t)stream, 0);
}

int rmpc_solve_batch_scene_device(rmpc_handle *h, int B, const rmpc_scene *scene, const double *d_xinit,
                                  const double *d_x0, double *d_z_out, int32_t *d_exitflag, int32_t *d_iters,
                                  double *d_kkt_res, double *d_obj, void *stream) {
  if (!h || !scene || !d_xinit || !d_x0 || !d_z_out || !d_exitflag || !d_iters || !d_kkt_res || !d_obj)
    return fail("null argument");
  if (rmpc_pack_scene_workspace(h, B, scene, stream)) return -1;
  return rmpc_solve_batch_packed_device(h, B, d_xinit, d_x0, d_z_out, d_exitflag, d_iters, d_kkt_res, d_obj, stream);
}

int rmpc_advance_device_flags(rmpc_handle *h, int B, const double *d_z_prev, const int32_t *d_exitflag, double *d_xinit,
                              double *d_x0, int previous_plan, void *stream) {
  if (!h || !d_z_prev || !d_xinit || !d_x0) return fail("null argument");
  if (B < 1 || B > h->max_batch) return fail("batch size out of range for this handle");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;   // NULL: the legacy null stream, ordered with the caller's default-stream work
  const int *ef = (const int *)d_exitflag;
  h->ops->advance(h, B, d_z_prev, ef, d_xinit, d_x0, previous_plan, st);
  HIPCHK(hipGetLastError());
  return 0;
}

int rmpc_advance_device(rmpc_handle *h, int B, const double *d_z_prev, double *d_xinit, double *d_x0,
                        int previous_plan, void *stream) {
  return rmpc_advance_device_flags(h, B, d_z_prev, nullptr, d_xinit, d_x0, previous_plan, stream);
}

int rmpc_retarget_device(rmpc_handle *h, int B, const rmpc_retarget *r, void *stream) {
  if (!h || !r) return fail("null argument");
  if (r->struct_size != (int)sizeof(rmpc_retarget)) return fail("rmpc_retarget.struct_size mismatch");
  if (!r->xinit || !r->x0 || !r->goal || !r->goal_pool || !r->cursor || !r->dwell || !r->x_start) return fail("null argument");
  if (B < 1 || B > h->max_batch) return fail("batch size out of range for this handle");
  if (r->pool_len < 1) return fail("goal pool must hold at least one goal per instance");
  if (!h->desc.has_goal) return fail("the model has no GoalReaching objective");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  RetargetDev R;
  R.xinit = r->xinit; R.x0 = r->x0; R.goal = r->goal; R.exitflag = (const int *)r->exitflag; R.iters = (const int *)r->iters;
  R.pool = r->goal_pool; R.x_start = r->x_start; R.P = r->pool_len; R.lower = r->lower_limits; R.upper = r->upper_limits;
  R.cursor = (int *)r->cursor; R.dwell = (int *)r->dwell; R.failrun = (int *)r->failrun;
  R.tol = r->tol; R.settle_vel = r->settle_vel; R.settle_min_dwell = r->settle_min_dwell; R.max_dwell = r->max_dwell;
  R.fail_reset_after = r->fail_reset_after; R.counts = (long long *)r->counts;
  R.wmu = h->warm_mode ? (h->fused ? h->F.wmu : h->W.wmu) : nullptr;
  R.wmu_regoal = r->mu_regoal > 0.0 ? r->mu_regoal / kWarmKappa : 0.0;
  h->ops->retarget(h, B, R, st);
  HIPCHK(hipGetLastError());
  return 0;
}

int rmpc_advance_obstacles_device(int B, int nobst, double dt, double arena, double *d_obst_dyn, void *stream) {
  if (B < 1 || nobst < 1 || !d_obst_dyn) return fail("bad argument");
  const int n = B * nobst;
  hipLaunchKernelGGL(k_obst_advance, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_obst_dyn, n, dt, arena);
  HIPCHK(hipGetLastError());
  return 0;
}

static int grid_device(const void *p);

int rmpc_free_space_device(int B, int N, int P, int K, double max_radius, const double *d_points,
                           const double *d_seeds, double *d_planes, void *stream) {
  if (!d_points || !d_seeds || !d_planes) return fail("null argument");
  if (B < 1 || N < 1 || K < 1 || P < 1 || P > 64) return fail("free space decomposition: need 1 <= P <= 64 points, K >= 1");
  if (grid_device(d_points)) return -1;
  hipLaunchKernelGGL(k_fsd, dim3((B * N + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_points, d_seeds, d_planes,
                     B, N, P, K, max_radius);
  HIPCHK(hipGetLastError());
  return 0;
}

/* the global planner (rmpc_grid.hpp): no handle; each call runs on the device its first pointer lives on */
static int grid_device(const void *p) {
  hipPointerAttribute_t a;
  HIPCHK(hipPointerGetAttributes(&a, p));
  if (a.device < 0) return fail("not a device pointer");
  HIPCHK(hipSetDevice(a.device));
  return 0;
}
static bool grid_fits(long long a, long long b) { return a >= 0 && b >= 0 && (b == 0 || a <= INT_MAX / b); }
static int grid_check(int H, int W, int movement) {
  if (H < 1 || W < 1 || !grid_fits(H, W)) return fail("grid: need H, W >= 1");
  if (movement != 4 && movement != 8) return fail("grid: movement must be 4 or 8");
  return 0;
}

int rmpc_grid_inflate_device(int H, int W, double cell, double size_robot, double threshold, const double *d_grid,
                             double *d_out, void *stream) {
  if (!d_grid || !d_out) return fail("null argument");
  if (grid_check(H, W, 8) || grid_device(d_grid)) return -1;
  if (!(cell > 0.0) || !(size_robot >= 0.0)) return fail("grid inflate: need cell > 0, size_robot >= 0");
  const double kd = ceil(size_robot / cell);
  if (kd > (double)(H + W)) return fail("grid inflate: window larger than the map");
  hipLaunchKernelGGL(k_grid_inflate, dim3((H * W + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_grid, d_out, H, W,
                     (int)kd, threshold);
  HIPCHK(hipGetLastError());
  return 0;
}

int rmpc_grid_fields_device(int H, int W, const double *d_grid, int G, const int32_t *d_goal_cells, int movement,
                            double occ_threshold, double cost_factor, double *d_fields, int32_t *d_status,
                            int32_t *d_sweeps, void *stream) {
  if (!d_grid || !d_goal_cells || !d_fields || !d_status) return fail("null argument");
  if (grid_check(H, W, movement)) return -1;
  if (H * W > RMPC_GRID_MAX_CELLS)
    return fail("grid fields: " + std::to_string(H) + "x" + std::to_string(W) + " map exceeds RMPC_GRID_MAX_CELLS = " +
                std::to_string(RMPC_GRID_MAX_CELLS) + " cells (one field must fit in the LDS of a workgroup)");
  if (G < 1 || !grid_fits(G, (long long)H * W)) return fail("grid fields: need 1 <= G and G*H*W <= INT_MAX");
  if (!(cost_factor >= 0.0) || std::isinf(cost_factor)) return fail("grid fields: cost_factor must be finite and >= 0");
  if (grid_device(d_grid)) return -1;
  hipLaunchKernelGGL(k_grid_fields, dim3(G), dim3(kGridThreads), 0, (hipStream_t)stream, d_grid, H, W,
                     (const int *)d_goal_cells, movement, occ_threshold, cost_factor, d_fields, (int *)d_status,
                     (int *)d_sweeps);
  HIPCHK(hipGetLastError());
  return 0;
}

int rmpc_grid_paths_device(int H, int W, const double *d_grid, int G, const double *d_fields, const int32_t *d_goal_cells,
                           int B, const int32_t *d_start_cell, const int32_t *d_goal_index, int movement,
                           double occ_threshold, double cost_factor, int max_len, int32_t *d_path, int32_t *d_len,
                           void *stream) {
  if (!d_grid || !d_fields || !d_goal_cells || !d_start_cell || !d_goal_index || !d_path || !d_len) return fail("null argument");
  if (grid_check(H, W, movement)) return -1;
  if (G < 1 || !grid_fits(G, (long long)H * W)) return fail("grid paths: need 1 <= G and G*H*W <= INT_MAX");
  if (B < 1 || max_len < 1 || !grid_fits(B, max_len)) return fail("grid paths: need B, max_len >= 1 and B*max_len <= INT_MAX");
  if (!(cost_factor >= 0.0) || std::isinf(cost_factor)) return fail("grid paths: cost_factor must be finite and >= 0");
  if (grid_device(d_grid)) return -1;
  hipLaunchKernelGGL(k_grid_paths, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_grid, H, W, d_fields,
                     (const int *)d_goal_cells, G, (const int *)d_start_cell, (const int *)d_goal_index, B, movement,
                     occ_threshold, cost_factor, max_len, (int *)d_path, (int *)d_len);
  HIPCHK(hipGetLastError());
  return 0;
}

int rmpc_grid_cells_device(int B, const double *d_pos, int stride, int H, int W, double x0, double y0, double cell,
                           int32_t *d_cells, void *stream) {
  if (!d_pos || !d_cells) return fail("null argument");
  if (B < 1 || stride < 2 || !grid_fits(B, stride)) return fail("grid cells: need B >= 1, stride >= 2, B*stride <= INT_MAX");
  if (grid_check(H, W, 8) || grid_device(d_pos)) return -1;
  if (!(cell > 0.0)) return fail("grid cells: need cell > 0");
  hipLaunchKernelGGL(k_grid_cells, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_pos, stride, B, H, W, x0,
                     y0, cell, (int *)d_cells);
  HIPCHK(hipGetLastError());
  return 0;
}

int rmpc_follow_path_device(int B, const int32_t *d_path, const int32_t *d_len, int max_len, int32_t *d_idx,
                            const double *d_pos, int stride, int W, double x0, double y0, double cell, double threshold,
                            double *d_goal, void *stream) {
  if (!d_path || !d_len || !d_idx || !d_pos || !d_goal) return fail("null argument");
  if (B < 1 || max_len < 1 || !grid_fits(B, max_len)) return fail("follow path: need B, max_len >= 1 and B*max_len <= INT_MAX");
  if (stride < 2 || !grid_fits(B, stride) || W < 1) return fail("follow path: need stride >= 2, W >= 1");
  if (grid_device(d_path)) return -1;
  hipLaunchKernelGGL(k_follow_path, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const int *)d_path,
                     (const int *)d_len, max_len, (int *)d_idx, d_pos, stride, B, W, x0, y0, cell, threshold, d_goal);
  HIPCHK(hipGetLastError());
  return 0;
}

/* the lidar (rmpc_sense.hpp): no handle; each call runs on the device its first pointer lives on */
int rmpc_lidar_scan_device(int B, const rmpc_lidar *l, void *stream) {
  if (!l) return fail("null argument");
  if (l->struct_size != (int)sizeof(rmpc_lidar)) return fail("rmpc_lidar.struct_size mismatch");
  if (B < 1 || l->rays < 1) return fail("lidar: need B >= 1 and rays >= 1");
  if (l->pose_stride < 3) return fail("lidar: pose_stride must be >= 3 (x, y, heading)");
  if (l->nbox < 0 || l->ncircle < 0) return fail("lidar: negative shape count");
  if (!grid_fits(B, l->rays) || !grid_fits(B, l->pose_stride) || !grid_fits(l->nbox, 4) || !grid_fits(l->ncircle, 3))
    return fail("lidar: B*rays, B*pose_stride, nbox*4 and ncircle*3 must not exceed INT_MAX");
  if (!(l->range > 0.0) || std::isinf(l->range)) return fail("lidar: range must be positive and finite");
  if (!l->pose || !l->points || (l->nbox > 0 && !l->boxes) || (l->ncircle > 0 && !l->circles)) return fail("null argument");
  if (grid_device(l->pose)) return -1;
  const int n = B * l->rays;
  const double step = (l->angle_max - l->angle_min) / (double)l->rays;
  hipLaunchKernelGGL(k_lidar, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, l->pose, l->pose_stride, B,
                     l->rays, l->angle_min, step, l->range, l->offset_x, l->offset_y, l->height, l->boxes, l->nbox,
                     l->circles, l->ncircle, l->points, l->ranges);
  HIPCHK(hipGetLastError());
  return 0;
}

static int plan_points(int B, int N, const double *d_z_prev, int nvar, const int32_t *d_exitflag, const double *d_pose,
                       int pose_stride, int shift, int heading, double offset_x, double offset_y, double height,
                       double *d_points, void *stream) {
  if (!d_pose || !d_points) return fail("null argument");
  if (B < 1 || N < 1) return fail("plan points: need B, N >= 1");
  if (heading != 0 && heading != 1) return fail("plan points: heading must be 0 or 1");
  if (pose_stride < 3) return fail("plan points: pose_stride must be >= 3 (x, y, heading)");
  if (nvar < 3) return fail("plan points: nvar must be >= 3 (x, y, heading first)");
  if (!grid_fits(B, N) || !grid_fits(B, pose_stride) || !grid_fits((long long)B * N, nvar))
    return fail("plan points: B*N, B*pose_stride and B*N*nvar must not exceed INT_MAX");
  if (grid_device(d_z_prev ? (const void *)d_z_prev : (const void *)d_pose)) return -1;
  hipLaunchKernelGGL(k_plan_points, dim3((B * N + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_z_prev, nvar,
                     (const int *)d_exitflag, d_pose, pose_stride, B, N, shift, heading, offset_x, offset_y, height,
                     d_points);
  HIPCHK(hipGetLastError());
  return 0;
}

int rmpc_plan_points_device(int B, int N, const double *d_z_prev, int nvar, const int32_t *d_exitflag,
                            const double *d_pose, int pose_stride, double offset_x, double offset_y, double height,
                            double *d_points, void *stream) {
  return plan_points(B, N, d_z_prev, nvar, d_exitflag, d_pose, pose_stride, 0, 1, offset_x, offset_y, height, d_points,
                     stream);
}

/* fleet separation (rmpc_sense.hpp): no handle; each call runs on the device its first pointer lives on */
int rmpc_fleet_points_device(int B, int N, const double *d_z_prev, int nvar, const int32_t *d_exitflag,
                             const double *d_pose, int pose_stride, int heading, double offset_x, double offset_y,
                             double height, double *d_points, void *stream) {
  return plan_points(B, N, d_z_prev, nvar, d_exitflag, d_pose, pose_stride, 1, heading, offset_x, offset_y, height,
                     d_points, stream);
}

int rmpc_fleet_planes_device(int B, int N, const double *d_points, const double *d_radius, int K, double range,
                             int nobst, int slot0, double *d_planes, void *stream) {
  if (!d_points || !d_radius || !d_planes) return fail("null argument");
  if (B < 1 || N < 1) return fail("fleet planes: need B, N >= 1");
  if (K < 1 || K > rmpc::kFleetKMax) return fail("fleet planes: need 1 <= K <= 8");
  if (slot0 < 0 || nobst < 1 || slot0 > nobst - K) return fail("fleet planes: need 0 <= slot0 and slot0 + K <= nobst");
  if (!(range >= 0.0)) return fail("fleet planes: range must be >= 0 (+inf admits every robot)");
  if (!grid_fits(B, N) || !grid_fits((long long)B * N, nobst) || !grid_fits((long long)B * N * nobst, 4))
    return fail("fleet planes: B*N*nobst*4 must not exceed INT_MAX");
  if (grid_device(d_points)) return -1;
  const int nbt = (B + 255) / 256;
  hipLaunchKernelGGL(k_fleet_planes, dim3(nbt * N), dim3(256), 0, (hipStream_t)stream, d_points, d_radius, B, N, K,
                     range * range, nobst, slot0, d_planes);
  HIPCHK(hipGetLastError());
  return 0;
}

int rmpc_set_warm_start(rmpc_handle *h, int mode) {
  if (!h) return fail("null handle");
  h->warm_mode = mode ? 1 : 0;
  h->have_duals = false;
  return 0;
}

int rmpc_set_pass_budget(rmpc_handle *h, int passes) {
  if (!h) return fail("null handle");
  if (passes < 0) return fail("pass budget must be >= 0");
  h->pass_budget = passes;
  return 0;
}

int rmpc_is_fused(const rmpc_handle *h) { return (h && h->fused) ? 1 : 0; }
const char *rmpc_fused_kernel_name(const rmpc_handle *h) {
  if (!h || !h->fused) return "";
  return h->ops->arm_fused ? "k_fused_arm" : "k_fused";
}
int rmpc_is_async(const rmpc_handle *h) { return (h && (h->fused || h->pass_budget > 0)) ? 1 : 0; }

int rmpc_set_profiling(rmpc_handle *h, int enable) {
  if (!h) return fail("null handle");
  h->profiling = enable != 0;
  for (int i = 0; i < RMPC_NUM_KERNELS; i++) { h->prof_ms[i] = 0; h->prof_n[i] = 0; h->prof_bytes[i] = 0; }
  return 0;
}

int rmpc_get_profile(rmpc_handle *h, double *total_ms, int64_t *launches, double *total_alg_bytes,
                     int64_t *full_launch_bytes) {
  if (!h) return fail("null handle");
  const int64_t L = (int64_t)h->max_batch * h->M.N;
  for (int i = 0; i < RMPC_NUM_KERNELS; i++) {
    if (total_ms) total_ms[i] = h->prof_ms[i];
    if (launches) launches[i] = h->prof_n[i];
    if (total_alg_bytes) total_alg_bytes[i] = h->prof_bytes[i];
    if (full_launch_bytes)
      full_launch_bytes[i] = (i == K_SWEEP || i == K_STEP) ? L * h->lane_bytes[i]
                             : (i == K_RICCATI || i == K_FUSED) ? (int64_t)h->max_batch * h->lane_bytes[i]
                                                                : h->lane_bytes[i];
  }
  return 0;
}

int rmpc_last_passes(rmpc_handle *h) {
  if (!h) return -1;
  if (h->fused && h->last_passes < 0) {
    // the fused kernel counts on the device: the most passes any instance of the last launch needed
    if (hipSetDevice(h->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(h->h_passes, h->F.passes, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
      return -1;
    h->last_passes = *h->h_passes;
  }
  if (!h->fused && h->last_passes == -2) {
    // a solve enqueued without a host look: passes after which instances were still iterating, plus the one that
    // found them all stopped
    if (hipSetDevice(h->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    h->h_hist.resize(h->last_cap + 1);
    if (hipMemcpy(h->h_hist.data(), h->W.active_hist, sizeof(int) * h->last_cap, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    int p = 0;
    while (p < h->last_cap && h->h_hist[p] > 0) p++;
    h->last_passes = p < h->last_cap ? p + 1 : h->last_cap;
  }
  return h->last_passes;
}

/* development aid (builds with -DRMPC_STAMPS): per-block phase cycles of the last fused launch, 8 words per block */
#ifdef RMPC_STAMPS
int rmpc_debug_sweep_stamps(long long *out) { return sum_stamps(&VariantOps::sweep_stamps, out); }   // k_sweep's sections
#endif
#ifdef RMPC_RIC_STAMPS
int rmpc_debug_ric_stamps(long long *out) { return sum_stamps(&VariantOps::ric_stamps, out); }   // the recursion's phases
#endif
int rmpc_debug_fused_stamps(rmpc_handle *h, long long *out, int nblocks) {
  if (!h || !h->fused) return fail("no fused workspace");
  if (nblocks > fused_columns(h->max_batch)) return fail("too many blocks");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, h->F.stamps, sizeof(long long) * 8 * (size_t)nblocks, hipMemcpyDeviceToHost));
  return 0;
}

/* test aid: NaN patterns into everything a solve could read without having written it -- the LDS of every CU (blocks
 * that own all 160 KB of a CU, then 64 KB blocks, so that whatever offset a solver kernel's allocation starts at has
 * been covered), the scratch (private) memory the wavefronts spill to, and the handle's whole device workspace (all
 * bytes 0xff: NaN as a double, -1 as an int; stored multipliers and the parameters of rmpc_pack_scene_workspace are
 * thereby forgotten).  A test then shows that no result depends on what a kernel finds in any of them. */
__global__ __launch_bounds__(64) void k_poison_lds(double *sink, int nbytes) {
  extern __shared__ double pl[];
  const int n = nbytes / 8;
  for (int i = threadIdx.x; i < n; i += 64) pl[i] = __longlong_as_double(0x7ff8dead0000beefLL);
  __syncthreads();
  if (sink && threadIdx.x == 0 && blockIdx.x == 0) sink[0] = pl[n - 1];
}
__global__ __launch_bounds__(64) void k_poison_scratch(double *sink, int salt) {
  // 4 KB of private memory per lane, indexed at run time (so that it lives in scratch), filled with NaN patterns
  // (launched with 40 KB of LDS per block: four wavefronts per CU, like the solver kernels that spill)
  volatile double buf[512];
  for (int i = 0; i < 512; i++) buf[i] = __longlong_as_double(0x7ff8dead0000beefLL + i);
  if (sink && salt == 12345) sink[threadIdx.x] = buf[(salt + threadIdx.x) % 512];
}
int rmpc_debug_poison_lds(rmpc_handle *h) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  const int sizes[2] = {160 * 1024, 64 * 1024};
  for (int si = 0; si < 2; si++) {
    HIPCHK(hipFuncSetAttribute((const void *)k_poison_lds, hipFuncAttributeMaxDynamicSharedMemorySize, sizes[si]));
    for (int rep = 0; rep < 4; rep++)
      hipLaunchKernelGGL(k_poison_lds, dim3(4096), dim3(64), sizes[si], h->stream, (double *)nullptr, sizes[si]);
    HIPCHK(hipGetLastError());
  }
  for (int rep = 0; rep < 2; rep++) hipLaunchKernelGGL(k_poison_scratch, dim3(8192), dim3(64), 40 * 1024, h->stream, (double *)nullptr, rep);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(h->ws_base, 0xff, h->ws_bytes, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->have_duals = false;
  h->packed_B = 0;
  return 0;
}

int rmpc_debug_sweep(rmpc_handle *h, int B, const double *xinit, const double *x0, const double *params,
                     double *out_Q, double *out_q0, double *out_q1, double *out_rc, double *out_g, double *out_f) {
  if (!h) return fail("null handle");
  if (B < 1 || B > h->max_batch) return fail("batch size out of range for this handle");
  HIPCHK(hipSetDevice(h->device));
  if (ensure_staging(h) != 0) return -1;
  const DevModel &M = h->M;
  hipStream_t st = h->stream;
  HIPCHK(hipMemcpyAsync(h->d_xinit, xinit, sizeof(double) * B * M.nx, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(h->d_x0, x0, sizeof(double) * (size_t)B * M.N * M.nv, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(h->d_params, params, sizeof(double) * (size_t)B * M.N * M.npar, hipMemcpyHostToDevice, st));
  dim3 g1((B + 63) / 64, (M.N * M.npar + 63) / 64);
  hipLaunchKernelGGL(k_pack, g1, dim3(256), 0, st, h->d_params, h->W.p, B, M.N * M.npar, M.npar, M.N, h->Bp);
  dim3 g2((B + 63) / 64, (M.N * M.nv + 63) / 64);
  hipLaunchKernelGGL(k_pack, g2, dim3(256), 0, st, h->d_x0, h->W.z[0], B, M.N * M.nv, M.nv, M.N, h->Bp);
  hipLaunchKernelGGL(k_init, dim3((B + 255) / 256), dim3(256), 0, st, h->W, h->d_xinit, B, M.nx, M.mu0, 0);
  h->have_duals = false;
  {
    const int wm = h->warm_mode;
    h->warm_mode = 0;
    h->ops->pass(h, Phase{h->W, B}, 1, 0, st, K_SWEEP);
    h->warm_mode = wm;
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  // gather SoA -> instance-major on the host (debug path, not timed)
  const size_t S = (size_t)M.N * h->Bp;
  auto fetch = [&](const double *dptr, size_t slots, std::vector<double> &v) -> int {
    v.resize(S * slots);
    HIPCHK(hipMemcpy(v.data(), dptr, sizeof(double) * S * slots, hipMemcpyDeviceToHost));
    return 0;
  };
  std::vector<double> R, gr, part;
  const int nq = M.n, nv = M.nv;
  const RecLayout L = rec_layout(M);
  if (fetch(h->W.R, L.rs, R) || fetch(h->W.grow[1], M.nh > 0 ? M.nh : 1, gr)  /* first pass: cur = 0, written to buffer 1 */ ||
      fetch(h->W.part, P_COUNT, part))
    return -1;
  auto at = [&](const std::vector<double> &v, int slot, int k, int b) { return v[((size_t)slot * M.N + k) * h->Bp + b]; };
  auto rec = [&](int off, int k, int b) { return R[((size_t)b * M.N + k) * L.rs + off]; };
  for (int b = 0; b < B; b++)
    for (int k = 0; k < M.N; k++) {
      const size_t sb = (size_t)b * M.N + k;
      if (out_Q) {
        double *Q = out_Q + sb * nv * nv;
        for (int i = 0; i < nv * nv; i++) Q[i] = 0.0;
        int s = 0;
        for (int a = 0; a < nq; a++)
          for (int c = a; c < nq; c++) { double v = rec(L.q + s++, k, b); Q[a * nv + c] = v; Q[c * nv + a] = v; }
        for (int j = nq; j < nv; j++) Q[j * nv + j] = rec(L.dg + j - nq, k, b);
        if (M.ns)
          for (int j = 0; j < nv; j++)
            if (j != M.nx) { double v = rec(L.cs + j, k, b); Q[j * nv + M.nx] = v; Q[M.nx * nv + j] = v; }
      }
      for (int j = 0; j < nv; j++) {
        if (out_q0) out_q0[sb * nv + j] = rec(L.q0 + j, k, b);
        if (out_q1) out_q1[sb * nv + j] = rec(L.q1 + j, k, b);
      }
      if (out_rc) for (int j = 0; j < M.nx; j++) out_rc[sb * M.nx + j] = (k < M.N - 1) ? rec(L.rc + j, k, b) : 0.0;
      if (out_g) for (int j = 0; j < M.nh; j++) out_g[sb * M.nh + j] = at(gr, j, k, b);
      if (out_f) out_f[sb] = at(part, P_F, k, b);
    }
  return 0;
}

}  // extern "C"
