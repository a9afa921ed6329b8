// rmpc_solver.hpp -- what every kernel of the solver shares: the solver constants, the device workspace (Ws) and its
// indexing, the address-space types and a few small helpers.  Part of rmpc_kernels.hip (included there first, inside
// namespace rmpc); needs rmpc_model.hpp.

// solver constants (DESIGN.md, section "Algorithm")
constexpr double kTMin = 1e-2;
// warm start of the multipliers (rmpc_set_warm_start; oracle: ORC_WARM_*): mu = clamp(kappa * previous final mu),
// slacks pushed to kWarmTMin only, multipliers max(previous, mu / t)
constexpr double kWarmKappa = 1000.0;
constexpr double kWarmMuMin = 1e-6;
constexpr double kWarmTMin = 1e-4;
// (the fraction to the boundary is per model: Cfg::TAU)
// barrier restart on stalled steps (oracle: ORC_RS_IT, ORC_RS_N, ORC_RS_ALPHA, ORC_RS_MU, ORC_RS_DECAY)
constexpr int kRsIt = 8, kRsN = 3;
constexpr double kRsAlpha = 0.2, kRsMu = 1e-3, kRsDecay = 0.3;
constexpr int kSweepBlock = 64;     // threads per k_sweep / k_step block: one wavefront, so that small batches spread over all CUs
constexpr int kLsMax = 25;
constexpr int kLsGrow = 1;         // step-length memory: a line search starts this many halvings above the last accepted one
constexpr double kArmijo = 1e-4;
constexpr double kMuDiverged = 1e12;
constexpr double kCurvMu = 1e-2; // curvature terms only once the barrier parameter is this small
constexpr int kLsCurv = 2;        // trials granted to a step computed with constraint curvature
constexpr int kCurvFailMax = 2;   // consecutive curvature-step failures before Gauss-Newton is latched
constexpr int kCurvBackMax = 16;  // (diff-drive) longest run of iterations a failed curvature step switches the terms off
constexpr int kGroupedMin = 512;    // list length from which the grouped Riccati blocks are used
constexpr double kCompFrac = 0.3; // share of tol_comp the convergence test asks for (oracle: ORC_COMP_FRAC)
constexpr double kCsMin = 0.3;    // scaled curvature (oracle: ORC_CS_MIN, ORC_CS_CLEAN)
constexpr int kCsClean = 3;
constexpr double kAccFeas = 1e-6; // acceptable termination: feasibility / complementarity level
constexpr int kDenseDiv = 8;      // identity list while more than B / kDenseDiv instances iterate; below: compacted list,
                                  // and the survivors move to the compact workspace at the host's next look
constexpr int kMigrateMin = 1024; // batches smaller than this never migrate

enum Status : int { ST_ACTIVE = 100 };

enum Part : int { P_F = 0, P_TH, P_LOGS, P_RSTAT, P_REQ, P_RINEQ, P_RCOMP, P_SUMC, P_MINC, P_BAD, P_COUNT };

// Explicit address spaces for what the fused kernel addresses: pointers that travel through structs or are
// selected at run time are otherwise compiled to FLAT accesses, which count on both memory counters and so
// serialise global-memory and LDS waits.
typedef __attribute__((address_space(1))) double gdouble;   // global memory
typedef __attribute__((address_space(3))) double ldouble;   // LDS

// Device workspace (all pointers into one allocation).
struct Ws {
  int N, Bp;
  double *p;                      // [npar][N][Bp]
  double *z[2], *t[2], *lam[2], *nu[2];
  double *dz, *nunew;
  double *grow[2], *Jq[2];        // row values / FK-row gradients at the iterate of the same buffer index
  double *R;                      // [Bp][N][rs] stage records k_sweep -> k_riccati (layout: Cfg::R_*)
  int rs;
  double *gfa;
  double *KP;                     // [Bp][N][kps] per instance and stage: gains K | kff | cost-to-go P (dense) | p --
                                  // private to k_riccati, instance-major so that a wavefront moves a record in one request
  int kps;                        // record stride (doubles, multiple of 8)
  double *part;                   // [P_COUNT][N][Bp]
  double *gphi;                   // [N][Bp]
  unsigned long long *amin_p, *amin_d;  // [Bp] fraction-to-the-boundary step lengths (bits of a positive double)
  // per instance [Bp]
  double *mu, *rho, *phi0, *Dd, *fcur, *thcur, *logcur;
  double *mu_hold;                // barrier restart (inst_decide): the level mu is held at, 0 = none
  double *res_stat, *res_eq, *res_ineq, *res_comp, *obj;
  int *status, *iters, *ls, *cur, *newstep;
  int *redo, *force_gn, *gn_sticky, *curv_fail, *usedc, *stall;
  int *curv_skip, *curv_back;     // (diff-drive) curvature steps still to be skipped / length of the last skip (back-off)
  int *small_steps;               // barrier restart: accepted short steps in a row
  double *theta_mem, *theta_c;    // scaled curvature (Cfg::CSCALE): the scale the next curvature step starts from / of this iteration
  int *theta_clean, *theta_retry; // ... accepted curvature steps in a row without a retry / this iteration has retried
  int *ls0, *lsst;                // halvings the current line search started from / the next one starts from
  int *active_hist;               // [max_passes] instances still iterating after each pass
  int *act_idx, *n_act;           // compacted list of the instances still iterating, its length
  int *orig;                      // [Bp] compact workspace only: column -> instance of the caller's batch
  // multipliers of the last solve (warm start of the next one): [m][N][Bp], [nx][N][Bp], final barrier
  // parameter [Bp]
  double *wlam, *wnu, *wmu;
};

#define IDX(slot, k, b) (((size_t)(slot) * W.N + (size_t)(k)) * W.Bp + (size_t)(b))
// the same with the lane's (stage, instance) offset precomputed (k_sweep / k_step): uniform slot base + 32-bit lane offset
#define IDXL(slot) ((size_t)(slot) * SS + loff)
#define IDXL1(slot) ((size_t)(slot) * SS + loff1)

// stage-0 state := xinit (mpcModel.py:108 xinitidx), per-instance state reset
__device__ __forceinline__ double warm_mu(double wmu, double mu0) {
  double mu = kWarmKappa * wmu;
  if (mu < kWarmMuMin) mu = kWarmMuMin;
  if (mu > mu0) mu = mu0;
  return mu;
}


// 1/x for normal positive x: hardware estimate + two Newton steps (about 1 ulp; a full fp64 division costs three
// times as many instructions and the sweep performs one or two per constraint row)
__device__ __forceinline__ double frcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  double e = fma(-x, r, 1.0);
  r = fma(r, e, r);
  e = fma(-x, r, 1.0);
  return fma(r, e, r);
}

// x is formed where this statement stands, not later: an empty statement that reads x from a vector register.  The
// compiler keeps the statement in program order among the loads, stores and scheduling barriers around it, so a long
// accumulation chain (a sum or a maximum over the rows of a stage) advances row by row and only the accumulator stays
// alive, not every row's operands up to the point where the chain is finally run.  x is an input only: what the
// compiler knows of the value (that the result of an fmax is already canonical, say) is kept, and no instruction is
// emitted.  Empty in the host build (the constraint is the device's).
template <class T>
__device__ __forceinline__ void formed_here(const T &x) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : : "v"(x));
#else
  (void)x;
#endif
}

// "some test of this lane has failed", gathered test by test where the tests stand.  An int that is or-ed with
// comparisons lives as a lane mask in scalar registers anyway; formed_here() would force it into a vector register
// (a select per test).  Here the mask is the variable: each test is the comparison and one scalar or, held in place
// as a scalar operand, and any() is one select at the end.  A lane reads only its own bit, so the lanes a call leaves
// out do not matter.  The host build keeps the int.
struct LaneTests {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned long long m = 0;
  __device__ __forceinline__ void add(const bool failed) {
    m |= __builtin_amdgcn_ballot_w64(failed);
    asm volatile("" : : "s"(m));
  }
  __device__ __forceinline__ int any() const { return (int)__builtin_amdgcn_inverse_ballot_w64(m); }
#else
  int m = 0;
  __device__ __forceinline__ void add(const bool failed) { m |= (int)failed; }
  __device__ __forceinline__ int any() const { return m; }
#endif
};

// compile-time loop: fn(integral_constant<int, L>) ... fn(integral_constant<int, H-1>)
template <int L, class F, int... I>
__device__ __forceinline__ void for_range_impl(F &&fn, std::integer_sequence<int, I...>) {
  (fn(std::integral_constant<int, L + I>{}), ...);
}
template <int L, int H, class F>
__device__ __forceinline__ void for_range(F &&fn) {
  for_range_impl<L>(fn, std::make_integer_sequence<int, (H > L ? H - L : 0)>{});
}

// v moved between lanes by a DPP control word (quad permutations, row mirrors and rotations; the row broadcast of dpp_row_bcast below):
// full-rate vector moves, no LDS crossbar round trip.  Every lane a reader takes its value from must be active.  The quad
// permutations and row_half_mirror read only the 8 aligned lanes the reader belongs to, the row controls (row_newbcast)
// only the reader's 16-lane row, and the callers keep those busy together: the paths that use them run with whole
// wavefronts or whole halves (a half that sits a call out leaves no hole in the other half's two rows).  So the `old`
// operand of the move is never taken -- it is left undefined, with bound_ctrl, and no instruction is spent on setting it
// (a zero cost two v_mov_b32 per move).
template <int CTRL>
__device__ __forceinline__ double dpp_move(const double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// v of lane L of the reader's 16-lane row, in every lane of that row (row_newbcast:L, the one control that exists as a
// 64-bit move: one v_mov_b64_dpp).  With bound_ctrl and all rows and banks enabled `old` is never taken.
template <int L>
__device__ __forceinline__ double dpp_row_bcast(const double v) {
  static_assert(L >= 0 && L < 16, "dpp_row_bcast: lane of a 16-lane row");
  return __builtin_amdgcn_update_dpp(v, v, 0x150 + L, 0xF, 0xF, true);
}
