// rmpc_host.hip -- the host unit: the handle and everything that takes one (variant lookup, generated-view
// matching, workspace carving, profiling, the launch loop, the solver entries of the C ABI, setters, debug and test
// aids).  The descriptor checks and row tables are in rmpc_desc.hpp, the kernels that do not depend on a kernel
// variant in rmpc_batch.hpp, the entries without a handle (planner, lidar, fleet planes, ...) in rmpc_world.hip.  It
// reaches the kernels of a variant through the handle's entry of the variant table (VariantOps, rmpc_host.hpp), which
// the units built from rmpc_variants.hip fill while the library loads.
#include "rmpc_host.hpp"
#include "rmpc_desc.hpp"
#include "rmpc_batch.hpp"

static_assert(kDescLsMax == kLsMax, "rmpc_desc.hpp: the default of rmpc_desc.ls_max is the solver's kLsMax");

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

// What every entry that works on B instances of a handle begins with, behind its own argument checks: B is one the
// handle was created for, and the calls that follow go to the handle's device.
static int enter_batch(rmpc_handle *h, int B) {
  if (B < 1 || B > h->max_batch) return fail("batch size out of range for this handle");
  HIPCHK(hipSetDevice(h->device));
  return 0;
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
  if (enter_batch(h, B)) return -1;
  const DevModel &M = h->M;
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
    // (k_fused leaves the multipliers in the warm-start arrays only for a handle in warm-start mode; k_fused_arm always)
    h->have_duals = h->warm_mode || h->ops->arm_fused; h->duals_B = B;
    h->last_passes = -1;   // on the device (rmpc_last_passes fetches it)
    for (int i = 0; i < 5; i++) h->path[i] = -1;
    h->path[5] = 1;
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
  // rmpc_last_solve_path: what this loop enqueues, noted as it does (no device read beyond the looks it takes anyway)
  int *const path = h->path;
  path[0] = -1; path[1] = -1; path[2] = -1; path[3] = -1; path[5] = 0;
  path[4] = B <= kCompactWaveMax ? RMPC_PATH_COMPACT_WAVE : RMPC_PATH_COMPACT_BLOCK;
  int seen = B;   // length of the list (*W.n_act) as of the last host look; it never grows
  for (; pass < cap; pass++) {
    const int first = pass == 0;
    { ProfScope ps(h, st, K_SWEEP); h->ops->pass(h, ph, first, pass, st, K_SWEEP); }
    { ProfScope ps(h, st, K_RICCATI); h->ops->pass(h, ph, first, pass, st, K_RICCATI); }
    // (grouped: both instantiations were launched and the list length picks one on the device -- below kGroupedMin at
    //  the last look means the one-wave blocks from then on)
    path[3] = (h->ric_sel == RMPC_PATH_RIC_GROUPED && seen < kGroupedMin) ? RMPC_PATH_RIC_WAVE : h->ric_sel;
    if (first) path[2] = path[3];
    if (ph.B <= kCompactWaveMax) hipLaunchKernelGGL(k_compact_wave, dim3(1), dim3(64), 0, st, ph.W, ph.B, pass);
    else hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, st, ph.W, ph.B, pass);
    { ProfScope ps(h, st, K_STEP); h->ops->pass(h, ph, first, pass, st, K_STEP); }
    if (h->profiling) HIPCHK(hipGetLastError());   // per pass when profiling is on (otherwise once after the loop)
    if (!async && pass + 1 == next_check && max_passes_override <= 0) {
      HIPCHK(hipMemcpyAsync(h->h_active, h->W.active_hist + pass, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      const int n = *h->h_active;
      if (n == 0) { pass++; break; }
      seen = n * kDenseDiv > ph.B ? ph.B : n;   // (k_compact: the identity list while most of the columns iterate)
      if (may_migrate && !migrated && n * kDenseDiv <= B) {
        // k_compact has just left the compacted list of the n survivors in the batch's workspace
        hipLaunchKernelGGL(k_migrate, dim3((n + 63) / 64, M.N), dim3(64), 0, st, h->W, h->Wc, n, M.nv, M.m, M.nx, M.npar,
                           M.nh, M.nfk * M.n);
        ph = Phase{h->Wc, n};
        migrated = true;
        path[0] = pass + 1; path[1] = n;
        seen = n;
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
static int sum_stamps(const int which, long long *out) {
  std::vector<int (*)(int, long long *)> seen;
  for (int i = 0; i < 8; i++) out[i] = 0;
  for (const VariantOps &v : variant_table()) {
    int (*const r)(int, long long *) = v.read_stamps;
    bool dup = false;
    for (auto q : seen) dup = dup || q == r;
    if (dup) continue;
    seen.push_back(r);
    long long part[8];
    if (r(which, part)) return 1;
    for (int i = 0; i < 8; i++) out[i] += part[i];
  }
  return 0;
}
#endif

// stage records -> the dense blocks of rmpc_debug_sweep / rmpc_debug_step in instance-major order; rec(off, k, b): word
// off of the record of stage k of instance b
// out_C (may be null): the curvature entries of the records as the dense symmetric matrix a recursion subtracts per
// unit weight -- R_C over the q block; the unicycle's R_D entries over (theta, omega, u1 | v, u0) in the order
// Cfg::ND lists them, placed here by variable index (not through RicCtx::cp).
template <class RecFn>
static void unpack_records(const DevModel &M, int B, RecFn rec, double *out_Q, double *out_q0, double *out_q1, double *out_rc,
                           double *out_C = nullptr) {
  const int nq = M.n, nv = M.nv;
  const RecLayout L = rec_layout(M);
  for (int b = 0; b < B; b++)
    for (int k = 0; k < M.N; k++) {
      const size_t sb = (size_t)b * M.N + k;
      if (out_C) {
        double *Cm = out_C + sb * nv * nv;
        for (int i = 0; i < nv * nv; i++) Cm[i] = 0.0;
        int s = 0;
        for (int a = 0; a < nq; a++)
          for (int c = a; c < nq; c++) { double v = rec(L.c + s++, k, b); Cm[a * nv + c] = v; Cm[c * nv + a] = v; }
        if (M.robot == RMPC_ROBOT_DIFFDRIVE) {
          const int th = 2, v_ = 6, om = 7, u0 = M.nx + M.ns, u1 = u0 + 1;
          const int pr[11][2] = {{th, om}, {th, u1}, {om, om}, {om, u1}, {u1, u1},
                                 {th, v_}, {th, u0}, {om, v_}, {om, u0}, {u1, v_}, {u1, u0}};
          for (int i = 0; i < 11; i++) {
            const double v = rec(L.d + i, k, b);
            Cm[pr[i][0] * nv + pr[i][1]] = v; Cm[pr[i][1] * nv + pr[i][0]] = v;
          }
        }
      }
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
    }
}

// rmpc_debug_wave_reduce (test aid): one wavefront runs the whole-horizon reductions of rmpc_inst.hpp over the caller's
// lane values, once with the shuffle exchanges and once with the vector-move exchanges the kernels use
// (tests/test_gpu_wave_reduce.py)
constexpr int kWaveReduceWords = 10;   // words per lane: the most a call of the kernels reduces together
template <int LPI, bool DPP>
__device__ void wave_reduce_debug(const int op, const double (&v)[kWaveReduceWords], double *out) {
  const int lane = threadIdx.x;
  double r[kWaveReduceWords];
  for (int w = 0; w < kWaveReduceWords; w++) r[w] = 0.0;
  if (op == 0) r[0] = wave_sum<LPI, DPP>(v[0]);
  else if (op == 1) r[0] = wave_max<LPI, DPP>(v[0]);
  else if (op == 2) r[0] = wave_min<LPI, DPP>(v[0]);
  else if (op == 3) {
    // the partials of a sweep: five sums, four maxima, one minimum
    double rs5[5] = {v[0], v[1], v[2], v[3], v[4]}, rm4[4] = {v[5], v[6], v[7], v[8]}, rn1[1] = {v[9]};
    wave_reduce_many<LPI, DPP>(rs5, rm4, rn1);
    for (int i = 0; i < 5; i++) r[i] = rs5[i];
    for (int i = 0; i < 4; i++) r[5 + i] = rm4[i];
    r[9] = rn1[0];
  } else {
    // the step lengths: one sum, no maximum (the kernels pass a constant zero in its place), two minima
    double rs1[1] = {v[0]}, rm0[1] = {0.0}, rn2[2] = {v[1], v[2]};
    wave_reduce_many<LPI, DPP>(rs1, rm0, rn2);
    r[0] = rs1[0]; r[1] = rn2[0]; r[2] = rn2[1]; r[3] = rm0[0];
  }
  for (int w = 0; w < kWaveReduceWords; w++) out[w * 64 + lane] = r[w];
}
__global__ __launch_bounds__(64) void k_wave_reduce_debug(const int lpi, const int op, const double *in, double *out_shfl, double *out_dpp) {
  // (lpi and op are uniform: every branch is taken by the whole wavefront)
  double v[kWaveReduceWords];
  for (int w = 0; w < kWaveReduceWords; w++) v[w] = in[w * 64 + threadIdx.x];
  if (lpi == 32) {
    wave_reduce_debug<32, XCHG_SHFL>(op, v, out_shfl);
    wave_reduce_debug<32, XCHG_DPP>(op, v, out_dpp);
  } else {
    wave_reduce_debug<64, XCHG_SHFL>(op, v, out_shfl);
    wave_reduce_debug<64, XCHG_DPP>(op, v, out_dpp);
  }
}
extern "C" {

int rmpc_version(void) { return RMPC_VERSION; }
#ifndef RMPC_SOURCE_HASH
#define RMPC_SOURCE_HASH "unhashed"
#endif
const char *rmpc_source_hash(void) { return RMPC_SOURCE_HASH; }
const char *rmpc_last_error(void) { return g_err.c_str(); }
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
  h->path[5] = h->fused ? 1 : 0;
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
  if (enter_batch(h, B)) return -1;
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
  if (enter_batch(h, B)) return -1;
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
  if (enter_batch(h, B)) return -1;
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
  if (enter_batch(h, B)) return -1;
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
  if (enter_batch(h, B)) return -1;
  if (r->pool_len < 1) return fail("goal pool must hold at least one goal per instance");
  if (!h->desc.has_goal) return fail("the model has no GoalReaching objective");
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

/* test aid: see include/rmpc.h */
int rmpc_last_solve_path(const rmpc_handle *h, int32_t out[6]) {
  if (!h) return fail("null handle");
  if (!out) return fail("rmpc_last_solve_path: out is NULL");
  for (int i = 0; i < 6; i++) out[i] = h->path[i];
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
int rmpc_debug_sweep_stamps(long long *out) { return sum_stamps(STAMPS_SWEEP, out); }   // k_sweep's sections
#endif
#ifdef RMPC_RIC_STAMPS
int rmpc_debug_ric_stamps(long long *out) { return sum_stamps(STAMPS_RIC, out); }   // the recursion's phases
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

/* test aid: see k_wave_reduce_debug */
int rmpc_debug_wave_reduce(int device, int lpi, int op, const double *in, double *out_shfl, double *out_dpp) {
  if (lpi != 32 && lpi != 64) return fail("rmpc_debug_wave_reduce: 32 or 64 lanes per instance");
  if (op < 0 || op > 4) return fail("rmpc_debug_wave_reduce: op 0 sum, 1 max, 2 min, 3 many (5, 4, 1), 4 many (1, 0, 2)");
  if (!in || !out_shfl || !out_dpp) return fail("rmpc_debug_wave_reduce: null array");
  HIPCHK(hipSetDevice(device));
  const size_t bytes = sizeof(double) * kWaveReduceWords * 64;
  double *d = nullptr;
  HIPCHK(hipMalloc(&d, 3 * bytes));
  hipError_t e = hipMemcpy(d, in, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d + kWaveReduceWords * 64, 0, 2 * bytes);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_wave_reduce_debug, dim3(1), dim3(64), 0, 0, lpi, op, d, d + kWaveReduceWords * 64, d + 2 * kWaveReduceWords * 64);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out_shfl, d + kWaveReduceWords * 64, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_dpp, d + 2 * kWaveReduceWords * 64, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(std::string("rmpc_debug_wave_reduce: ") + hipGetErrorString(e));
  return 0;
}

int rmpc_debug_sweep(rmpc_handle *h, int B, const double *xinit, const double *x0, const double *params,
                     double *out_Q, double *out_q0, double *out_q1, double *out_rc, double *out_g, double *out_f) {
  if (!h) return fail("null handle");
  if (enter_batch(h, B)) return -1;
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
  const RecLayout L = rec_layout(M);
  if (fetch(h->W.R, L.rs, R) || fetch(h->W.grow[1], M.nh > 0 ? M.nh : 1, gr)  /* first pass: cur = 0, written to buffer 1 */ ||
      fetch(h->W.part, P_COUNT, part))
    return -1;
  auto at = [&](const std::vector<double> &v, int slot, int k, int b) { return v[((size_t)slot * M.N + k) * h->Bp + b]; };
  auto rec = [&](int off, int k, int b) { return R[((size_t)b * M.N + k) * L.rs + off]; };
  unpack_records(M, B, rec, out_Q, out_q0, out_q1, out_rc);
  for (int b = 0; b < B; b++)
    for (int k = 0; k < M.N; k++) {
      const size_t sb = (size_t)b * M.N + k;
      if (out_g) for (int j = 0; j < M.nh; j++) out_g[sb * M.nh + j] = at(gr, j, k, b);
      if (out_f) out_f[sb] = at(part, P_F, k, b);
    }
  return 0;
}

int rmpc_debug_step(rmpc_handle *h, int B, const double *xinit, const double *x0, const double *params,
                    const double *lam_w, const double *nu_w, const double *mu_w, double *out_Q, double *out_q0,
                    double *out_q1, double *out_rc, double *out_t, double *out_lam, double *out_mu, double *out_dz,
                    double *out_nu, int32_t *out_ok, int m_rows, int32_t *out_path) {
  return rmpc_debug_step_curv(h, B, xinit, x0, params, lam_w, nu_w, mu_w, out_Q, out_q0, out_q1, out_rc, out_t, out_lam, out_mu,
                              out_dz, out_nu, out_ok, m_rows, out_path, 0.0, nullptr);
}

int rmpc_debug_step_curv(rmpc_handle *h, int B, const double *xinit, const double *x0, const double *params,
                         const double *lam_w, const double *nu_w, const double *mu_w, double *out_Q, double *out_q0,
                         double *out_q1, double *out_rc, double *out_t, double *out_lam, double *out_mu, double *out_dz,
                         double *out_nu, int32_t *out_ok, int m_rows, int32_t *out_path, double cw, double *out_C) {
  if (!h || !xinit || !x0 || !params || !out_t || !out_lam || !out_mu || !out_dz || !out_nu || !out_ok) return fail("null argument");
  if (m_rows != h->M.m) return fail("rmpc_debug_step: out_t / out_lam are sized for " + std::to_string(m_rows) + " rows, the model has " + std::to_string(h->M.m));
  if (out_path) {
    // what the handle holds of the switches that select the path (read once, at rmpc_create)
    out_path[0] = h->fused ? (h->ops->arm_fused ? 2 : 1) : 0;
    out_path[1] = h->ric_lane;
    out_path[2] = (h->fused && h->ops->arm_fused) ? ((3 * h->M.N <= 64 && !h->env_arm_two_parts) ? 3 : 2) : 0;
    out_path[3] = h->ops->matches ? 1 : 0;
  }
  const int warm = (lam_w || nu_w || mu_w) ? 1 : 0;
  if (warm && !(lam_w && nu_w && mu_w)) return fail("rmpc_debug_step: lam_w, nu_w and mu_w come together");
  // the plain hook (cw = 0, no out_C) sweeps without the curvature terms, as it always has; the other sweeps with the model's
  const bool curv = cw != 0.0 || out_C != nullptr;
  const int sweep_curv = curv ? h->M.use_curv : 0;
  if (!(cw >= 0.0 && cw <= 1.0)) return fail("rmpc_debug_step_curv: the curvature weight is in [0, 1]");
  if (h->fused && h->ops->arm_fused && cw != 0.0 && cw != 1.0)
    return fail("rmpc_debug_step_curv: k_fused_arm runs its recursion at the weight 0 or 1");
  if (enter_batch(h, B)) return -1;
  if (ensure_staging(h) != 0) return -1;
  const DevModel &M = h->M;
  const int N = M.N, nv = M.nv, nx = M.nx, m = M.m;
  hipStream_t st = h->stream;
  HIPCHK(hipMemcpyAsync(h->d_xinit, xinit, sizeof(double) * B * nx, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(h->d_x0, x0, sizeof(double) * (size_t)B * N * nv, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(h->d_params, params, sizeof(double) * (size_t)B * N * M.npar, hipMemcpyHostToDevice, st));
  h->have_duals = false;
  h->packed_B = 0;
  const int rs = h->ops->rs;
  std::vector<double> R, tv, lv, dz, nn, mu((size_t)B);
  std::vector<int> ok((size_t)B);
  // word `slot` of stage k of instance b in an array of the workspace the handle's path runs in
  const size_t S32 = kFusedStages;
  const int fm = h->fused ? h->F.m : m;   // (the arms' fused workspace: one spare row behind the m rows)
  auto widx = [&](int slots, int slot, int k, int b) -> size_t {
    return h->fused ? ((size_t)b * slots + slot) * S32 + k : ((size_t)slot * N + k) * h->Bp + b;
  };
  if (warm) {
    // the multipliers of the "previous solve", in the layout k_save_duals / the fused epilogue leave them in
    const size_t cols = h->fused ? (size_t)fused_columns(h->max_batch) * S32 : (size_t)N * h->Bp;
    std::vector<double> wl(cols * fm, 0.0), wn(cols * nx, 0.0);
    for (int b = 0; b < B; b++)
      for (int k = 0; k < N; k++) {
        for (int i = 0; i < m; i++) wl[widx(fm, i, k, b)] = lam_w[((size_t)b * N + k) * m + i];
        for (int j = 0; j < nx; j++) wn[widx(nx, j, k, b)] = nu_w[((size_t)b * N + k) * nx + j];
      }
    HIPCHK(hipMemcpy(h->fused ? h->F.wlam : h->W.wlam, wl.data(), sizeof(double) * wl.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->fused ? h->F.wnu : h->W.wnu, wn.data(), sizeof(double) * wn.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->fused ? h->F.wmu : h->W.wmu, mu_w, sizeof(double) * B, hipMemcpyHostToDevice));
  }
  auto fetch = [&](const double *dptr, size_t n, std::vector<double> &v) -> int {
    v.resize(n);
    HIPCHK(hipMemcpy(v.data(), dptr, sizeof(double) * n, hipMemcpyDeviceToHost));
    return 0;
  };
  if (h->fused) {
    if (!h->ops->fused_step_debug) return fail("rmpc_debug_step: no debug kernel for this fused variant");
    double *d_buf = nullptr;
    int *d_ok = nullptr;
    const size_t n_rec = (size_t)B * N * rs, n_dz = (size_t)B * N * nv, n_nu = (size_t)B * N * nx;
    HIPCHK(hipMalloc((void **)&d_buf, sizeof(double) * (n_rec + n_dz + n_nu + B)));
    if (hipMalloc((void **)&d_ok, sizeof(int) * B) != hipSuccess) { (void)hipFree(d_buf); return fail("hipMalloc"); }
    double *const d_rec = d_buf, *const d_dz = d_rec + n_rec, *const d_nu = d_dz + n_dz, *const d_mu = d_nu + n_nu;
    hipError_t e = hipMemsetAsync(d_buf, 0, sizeof(double) * (n_rec + n_dz + n_nu + B), st);
    if (e == hipSuccess) {
      h->ops->fused_step_debug(h, B, h->d_xinit, h->d_x0, h->d_params, warm, sweep_curv, cw, d_rec, d_dz, d_nu, d_mu, d_ok, st);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    R.resize(n_rec); dz.resize(n_dz); nn.resize(n_nu);
    if (e == hipSuccess) e = hipMemcpy(R.data(), d_rec, sizeof(double) * n_rec, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(dz.data(), d_dz, sizeof(double) * n_dz, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(nn.data(), d_nu, sizeof(double) * n_nu, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(mu.data(), d_mu, sizeof(double) * B, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(ok.data(), d_ok, sizeof(int) * B, hipMemcpyDeviceToHost);
    (void)hipFree(d_buf);
    (void)hipFree(d_ok);
    if (e != hipSuccess) return fail(std::string("rmpc_debug_step: ") + hipGetErrorString(e));
    // the first sweep writes the trial point's slacks and multipliers to buffer 1 (cur = 0)
    const size_t cols = (size_t)fused_columns(h->max_batch) * S32;
    if (fetch(h->F.t[1], cols * fm, tv) || fetch(h->F.lam[1], cols * fm, lv)) return -1;
    for (int b = 0; b < B; b++)
      for (int k = 0; k < N; k++) {
        const size_t sb = (size_t)b * N + k;
        for (int j = 0; j < nv; j++) out_dz[sb * nv + j] = dz[sb * nv + j];
        for (int j = 0; j < nx; j++) out_nu[sb * nx + j] = k ? nn[sb * nx + j] : 0.0;   // (no path forms the costate of the fixed first state)
      }
  } else {
    dim3 g1((B + 63) / 64, (N * M.npar + 63) / 64);
    hipLaunchKernelGGL(k_pack, g1, dim3(256), 0, st, h->d_params, h->W.p, B, N * M.npar, M.npar, N, h->Bp);
    dim3 g2((B + 63) / 64, (N * nv + 63) / 64);
    hipLaunchKernelGGL(k_pack, g2, dim3(256), 0, st, h->d_x0, h->W.z[0], B, N * nv, nv, N, h->Bp);
    hipLaunchKernelGGL(k_init, dim3((B + 255) / 256), dim3(256), 0, st, h->W, h->d_xinit, B, nx, M.mu0, warm);
    int *d_okp = nullptr;   // (rmpc_debug_step_curv) the recursion's return value / lane path: the weight cannot be taken
    int lane_path = 0;
    if (curv) HIPCHK(hipMalloc((void **)&d_okp, sizeof(int) * B));
    {
      // the existing first pass, cold or warm: k_sweep (plain hook: with the curvature terms off), then the recursion
      // kernel, or the recursion at the weight cw
      const int wm = h->warm_mode, uc = h->M.use_curv;
      h->warm_mode = warm; h->have_duals = warm != 0; h->M.use_curv = sweep_curv;
      h->ops->pass(h, Phase{h->W, B}, 1, 0, st, K_SWEEP);
      if (curv) lane_path = h->ops->pass_step_debug(h, Phase{h->W, B}, cw, d_okp, st);
      else h->ops->pass(h, Phase{h->W, B}, 1, 0, st, K_RICCATI);
      h->warm_mode = wm; h->have_duals = false; h->M.use_curv = uc;
    }
    std::vector<int> okp((size_t)(curv ? B : 0));
    {
      hipError_t e = hipStreamSynchronize(st);
      if (e == hipSuccess) e = hipGetLastError();
      if (e == hipSuccess && curv) e = hipMemcpy(okp.data(), d_okp, sizeof(int) * B, hipMemcpyDeviceToHost);
      if (d_okp) (void)hipFree(d_okp);
      if (e != hipSuccess) return fail(std::string("rmpc_debug_step: ") + hipGetErrorString(e));
    }
    if (lane_path)
      for (int b = 0; b < B; b++)
        if (okp[b])
          return fail("rmpc_debug_step_curv: k_riccati_lane takes its curvature weight from the instance (mu <= 1e-2: the scale, "
                      "else 0); this first pass cannot run at the weight asked for");
    const size_t S = (size_t)N * h->Bp;
    std::vector<int> newstep((size_t)B), status((size_t)B);
    if (fetch(h->W.R, S * rs, R) || fetch(h->W.t[1], S * m, tv) || fetch(h->W.lam[1], S * m, lv) || fetch(h->W.dz, S * nv, dz) ||
        fetch(h->W.nunew, S * nx, nn) || fetch(h->W.mu, (size_t)B, mu))
      return -1;
    HIPCHK(hipMemcpy(newstep.data(), h->W.newstep, sizeof(int) * B, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(status.data(), h->W.status, sizeof(int) * B, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; b++) {
      if (curv && !lane_path) ok[b] = okp[b];
      else ok[b] = (status[b] == ST_ACTIVE && newstep[b] == 1) ? 1 : 0;   // (what the kernel stores when the recursion returned true)
      for (int k = 0; k < N; k++) {
        const size_t sb = (size_t)b * N + k;
        for (int j = 0; j < nv; j++) out_dz[sb * nv + j] = dz[widx(nv, j, k, b)];
        for (int j = 0; j < nx; j++) out_nu[sb * nx + j] = k ? nn[widx(nx, j, k, b)] : 0.0;
      }
    }
  }
  auto rec = [&](int off, int k, int b) { return R[((size_t)b * N + k) * rs + off]; };
  unpack_records(M, B, rec, out_Q, out_q0, out_q1, out_rc, out_C);
  for (int b = 0; b < B; b++) {
    out_mu[b] = mu[b];
    out_ok[b] = ok[b];
    for (int k = 0; k < N; k++)
      for (int i = 0; i < m; i++) {
        out_t[((size_t)b * N + k) * m + i] = tv[widx(fm, i, k, b)];
        out_lam[((size_t)b * N + k) * m + i] = lv[widx(fm, i, k, b)];
      }
  }
  return 0;
}

}  // extern "C"
