// rmpc_batch.hpp -- the solver kernels that do not depend on a kernel variant: they work on the batch workspace (Ws)
// whatever the robot -- pack / unpack between the ABI layout and the workspace, k_init, the warm-start copy, the list
// of iterating instances, the migration to the compact workspace, the launch order of a fused launch and the scene
// packer.  Included by rmpc_host.hip only, behind rmpc_kernels.hip (rmpc_solver.hpp: Ws, IDX, ST_ACTIVE, warm_mu, ...).
#pragma once

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

}  // namespace rmpc
