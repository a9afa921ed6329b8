// rmpc_kernels.hip -- batched multiple-shooting interior-point MPC solver for
// MI355X (gfx950).  Replaces the FORCES Pro generated solver behind
// robotmpcs.planner.mpcPlanner.MPCPlanner.solve() (mpcPlanner.py:262).
//
// One solve = pack, then passes of three kernels until every instance has
// stopped, then unpack:
//
//   k_sweep   one lane per (instance, stage): forms the trial point
//             z + alpha dz (t, lambda, nu likewise), evaluates dynamics, cost,
//             inequality rows and their Jacobians there, condenses the barrier
//             terms into the stage record (Hessian / gradient blocks) and writes
//             the merit and KKT partial sums of the stage.   [HBM / request bound]
//   k_riccati one wavefront per instance, stage matrices in LDS: reduces the
//             stage partials, runs the Armijo test on the l1 merit, updates the
//             barrier parameter, checks convergence and runs the block-
//             tridiagonal Riccati recursion (backward, forward, costates).
//                                    [LDS throughput / LDS round-trip latency]
//   k_step    one lane per (instance, stage): fraction-to-the-boundary partial
//             minima of the slack and multiplier steps, merit slope partials.
//                                                                  [HBM bound]
//   (+ k_compact: list of the instances still iterating; k_migrate: their move
//    to a small dense workspace once few are left)
//
// Data layout: what the stage-parallel kernels exchange is [slot][stage][instance]
// with the instance index contiguous (a wavefront's 64 lanes move 512 contiguous
// bytes per slot); what the wave-per-instance kernel reads or keeps is
// [instance][stage][record] (one request per record).  Iterates are double
// buffered per instance (cur / cur^1): a trial point is written once and
// accepted by flipping a bit.  DESIGN.md, sections 4 and 5.
//
// This file holds the device code that both kinds of translation unit include:
// rmpc_variants.hip instantiates the kernel templates of some kernel variants,
// rmpc_host.hip adds the kernels that do not depend on a variant (pack, unpack,
// compaction, migration, scene packing, ...) and the host side.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "rmpc_model.hpp"
#include "rmpc_spec_gen.hpp"   // generated views of the shipped configurations (scripts/gen_specs.py)

namespace rmpc {

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

// compile-time loop: fn(integral_constant<int, L>) ... fn(integral_constant<int, H-1>)
template <int L, class F, int... I>
__device__ __forceinline__ void for_range_impl(F &&fn, std::integer_sequence<int, I...>) {
  (fn(std::integral_constant<int, L + I>{}), ...);
}
template <int L, int H, class F>
__device__ __forceinline__ void for_range(F &&fn) {
  for_range_impl<L>(fn, std::make_integer_sequence<int, (H > L ? H - L : 0)>{});
}

// ===========================================================================
// k_sweep: stage-parallel function / Jacobian evaluation + condensing
// ===========================================================================
// Rows are processed in two groups so that every register array is indexed by an
// unrolled loop counter only and loads can be issued in batches:
//   * FK rows (distance / plane rows), grouped by kinematic slot (static slot loop,
//     short runtime loop over the rows of the slot);
//   * single-variable rows (limits and simple bounds), grouped by variable (static
//     loops; absent entries load row 0 and are masked -- a branch around a load,
//     even a wave-uniform one, makes hipcc wait for every element separately).

// Step lengths of one stage (k_step's arithmetic): the fraction-to-the-boundary minima over the rows and the merit
// slope partial.  One copy of the row code for step_body and for the merged form inside sweep_body (PHASE 1): the
// callers differ in where the inputs come from, not in what is done with them.
template <class C>
struct StepRow {
  double ap = 1.0, ad = 1.0, gphi = 0.0;
  template <int NV_>
  __device__ __forceinline__ void slope(const double (&gfv)[NV_], const double (&dz)[NV_]) {
#pragma unroll
    for (int j = 0; j < NV_; j++) gphi += gfv[j] * dz[j];
  }
  __device__ __forceinline__ void row(const double mu, const double gdz, const double g, const double tv, const double lv) {
    const double dt = gdz + (g - tv);
    const double itv = frcp(tv);
    const double dl = (mu - tv * lv - lv * dt) * itv;   // (same expression as in sweep_body's row_core)
    // the steps themselves are not kept: the sweep recomputes them from the same inputs
    // ratio tests with Newton reciprocals (the quotient of a non-negative step is discarded by the select)
    const double rp = -C::TAU * tv * frcp(dt), rd = -C::TAU * lv * frcp(dl);
    // (bitwise and: no short-circuit branch -- the rows of a stage stay one basic block)
    ap = ((dt < 0) & (rp < ap)) ? rp : ap;
    ad = ((dl < 0) & (rd < ad)) ? rd : ad;
    gphi -= mu * dt * itv;
  }
  // distance row r: jq = its gradient at the current iterate
  template <class V, int NV_>
  __device__ __forceinline__ void fk_row(const double mu, const double (&dz)[NV_], const double g, const double tv, const double lv,
                                         const double (&jq)[C::NQ]) {
    double gdz = 0.0;
#pragma unroll
    for (int a = 0; a < C::NQ; a++) gdz += jq[a] * dz[a];
    if constexpr (C::NS > 0) gdz += dz[C::NX];
    row(mu, gdz, g, tv, lv);
  }
  // single-variable row (j, u) (present: v_row(j, u) >= 0); gl: its stored value (general rows only)
  template <class V, int NV_>
  __device__ __forceinline__ void var_row(const V &v, const int k, const double mu, const int j, const int u, const double (&z)[NV_],
                                          const double (&dz)[NV_], const double gl, const double tv, const double lv) {
    const bool general = v.v_poff(j, u) >= 0;
    const double gvv = general ? gl : ((k == 0 && j < C::NX) ? 1.0 : (double)v.v_sgn(j, u) * (z[j] - v.v_val(j, u)));
    double gdz = (double)v.v_sgn(j, u) * dz[j];
    if constexpr (C::NS > 0) { if (v.v_soft(j, u)) gdz += dz[C::NX]; }
    row(mu, gdz, gvv, tv, lv);
  }
};

// inputs of a distance row of the sweep: slack, multiplier, value and gradient at the current iterate, obstacle, weight
template <int NQ_>
struct SweepFkBuf { double tcv, lcv, gold, jo[NQ_], op[4], wi; };
// What sweep_body requests at its top, before the trial point can be formed.  A local of the body; the merged call of
// the fused kernel (PHASE 1 / 2) keeps it in registers across the reduction of the step lengths, together with the
// slacks and multipliers of the single-variable rows (vt, vl: otherwise requested two variables ahead of their rows).
template <class C, class V>
struct SweepTop {
  static constexpr int NFKC = []() { if constexpr (V::SPEC) return V::nfkrows() > 0 ? V::nfkrows() : 1; else return 1; }();
  double zo[C::NV], dzo[C::NV];   // current iterate and step of this stage (the row steps are recomputed from them)
  double x1[C::NX], dx1[C::NX], n0[C::NX], n0n[C::NX], n1[C::NX], n1n[C::NX];
  double wuv[C::NU], wsv, rbody, goalv[3], wgoalv[3];
  SweepFkBuf<C::NQ> fkb[NFKC];
  double vt[C::NV][kVarRows], vl[C::NV][kVarRows];
};

// What one lane -- one (instance, stage) pair -- of the stage-parallel sweep addresses.  Element `slot` of an
// array is ptr[slot * SS + loff]: the batch-minor SoA of the pass kernels (SS = N * Bp, loff = k * Bp + b,
// next stage kstride = Bp) and the per-instance layout of the fused kernel ([instance][slot][32 stages]:
// SS = 32, loff = k, kstride = 1, pointers advanced to the instance) run the same code.
template <class RP = gdouble, class SP = RP>   // RP / SP: where the stage record / the step live (gdouble, or ldouble in the fused kernels)
struct SweepIO {
  const gdouble *zc, *tc, *lc, *nc, *pp, *gro, *jqo;   // iterate (current buffer), parameters
  gdouble *zn, *tn, *ln, *nn, *grn, *jqn, *gfa;        // trial point (other buffer), cost gradient
  const SP *dzp, *nup;                                 // step
  RP *rec;                                             // this lane's stage record
  size_t SS;
  unsigned loff, kstride;
  // the step (dzp, nup) may live elsewhere (fused kernel: in the LDS slots of the instance): own strides
  size_t SSd;
  unsigned loffd, kstrided;
  // first pass of a warm-started solve: multipliers / costates of the previous solve (same addressing as lc / nc;
  // stage k takes the values of stage k + 1, like the shifted plan)
  const gdouble *wl, *wn;
  int warm;
};
// merit / KKT partial sums of one stage (order = enum Part)
struct Partials {
  double f, th, logs, rstat, req, rineq, rcomp, sumc, minc, bad;
#ifdef RMPC_STAMPS
  long long tk[6];   // development builds: cycles of the sections of the sweep ([4], [5]: step lengths and their reduction, fused_sweep_step_call)
#endif
};

// Development aid (builds with -DRMPC_STAMPS): cycle stamps of the sweeps and of the fused kernels' pass loops.  Like
// RicStamps (rmpc_riccati.hpp) the recorders have a body in those builds and none otherwise, so the places that
// stamp carry no #ifdef and a production build is the code without them.
enum StampPhase { PH_SWEEP = 0, PH_DEC = 1, PH_RIC = 2, PH_STEP = 3 };   // words 0 .. 3 of a wavefront's record
#ifdef RMPC_STAMPS
// cycles per section of k_sweep / of the arms' sweep call, summed over the wavefronts of all launches
// (static: one copy per translation unit, read through the unit's entries of the variant table)
static __device__ long long g_sst[8];
// Sections of a sweep: st(i) adds the cycles since the previous stamp to section i.
struct SecStamps {
  long long acc[8], t0;
  __device__ __forceinline__ void start() {
    for (int i = 0; i < 8; i++) acc[i] = 0;
    t0 = __builtin_amdgcn_s_memtime();
  }
  __device__ __forceinline__ void operator()(const int i) {
    const long long t = __builtin_amdgcn_s_memtime();
    acc[i] += t - t0;
    t0 = t;
  }
  // sections i0 .. i0 + n - 1 into / out of the tk words of a Partials or a SweepStepOut
  template <class O>
  __device__ __forceinline__ void put(O &o, const int i0, const int n) const {
    for (int i = i0; i < i0 + n; i++) o.tk[i] = acc[i];
  }
  template <class O>
  __device__ __forceinline__ void get(const O &o, const int i0, const int n) {
    for (int i = i0; i < i0 + n; i++) acc[i] = o.tk[i];
  }
  // the first n sections and a call into g_sst (lane0: one lane of the wavefront)
  __device__ __forceinline__ void flush(const bool lane0, const int n) {
    if (lane0) {
      for (int i = 0; i < n; i++) atomicAdd((unsigned long long *)&g_sst[i], (unsigned long long)acc[i]);
      atomicAdd((unsigned long long *)&g_sst[7], 1ull);
    }
  }
};
// The pass loop of k_fused / k_fused_arm: cycles per phase, event counters and the wavefront's 8-word record in
// FusedWs::stamps (read by scripts/fused_stamps.py and tests/tools/dev_arm_fused_stamps.py).
struct PassStamps {
  long long ph[4], sec[8], hand, t_start, t_a, t_top, t_sub;
  int pass, ipass, nhand, both;
  __device__ __forceinline__ void start() {
    for (int i = 0; i < 4; i++) ph[i] = 0;
    for (int i = 0; i < 8; i++) sec[i] = 0;
    hand = 0;
    pass = ipass = nhand = both = 0;
    t_start = t_a = __builtin_amdgcn_s_memtime();
  }
  // hand-over: from the top of the pass loop to the test that ends it; events = epilogues + prologues (their lane 0)
  __device__ __forceinline__ void hand_begin() { t_top = __builtin_amdgcn_s_memtime(); }
  __device__ __forceinline__ void hand_events(const bool left, const bool took) {
    nhand += __popcll(__ballot(left)) + __popcll(__ballot(took));
  }
  __device__ __forceinline__ void hand_end() { hand += __builtin_amdgcn_s_memtime() - t_top; }
  // a pass of the wavefront.  inst: lane 0 of every instance that takes the pass; v1: the lane runs the first-pass copy
  // of the sweep call (both copies run when the two halves of k_fused differ)
  __device__ __forceinline__ void pass_begin(const bool inst, const bool v1) {
    pass++;
    ipass += __popcll(__ballot(inst));
    both += (__ballot(v1) != 0ull && __ballot(!v1) != 0ull) ? 1 : 0;
  }
  __device__ __forceinline__ void mark() { t_a = __builtin_amdgcn_s_memtime(); }
  // the cycles since the previous stamp (or mark) belong to phase p
  __device__ __forceinline__ void operator()(const int p) {
    const long long t = __builtin_amdgcn_s_memtime();
    ph[p] += t - t_a;
    t_a = t;
  }
  // k_fused, inside the sweep phase: the sections of the sweep call (lane 0's instance), then [6] unpark + reductions
  // and [7] the ordering point's wait.  (By value: a reference to the caller's partials among the arguments, even of an
  // empty function, changes how production code schedules their initialisation.)
  template <class O>
  __device__ __forceinline__ void sections(const O o) {
    for (int i = 0; i < 6; i++) sec[i] += __builtin_amdgcn_readfirstlane((int)o.tk[i]);
  }
  __device__ __forceinline__ void sweep_returned() { t_sub = __builtin_amdgcn_s_memtime(); }
  __device__ __forceinline__ void sweep_reduced() {
    const long long t = __builtin_amdgcn_s_memtime();
    sec[6] += t - t_sub;
    t_sub = t;
  }
  __device__ __forceinline__ void sweep_end() {
    (*this)(PH_SWEEP);
    sec[7] += t_a - t_sub;
  }
  // Record of the wavefront: [0 .. 3] phases, [4] total, [5] passes | passes with both sweep copies << 32,
  // [7] instance passes | hand-over events << 32.  k_fused (two = true): [6] hand-over cycles, and the sections as a
  // second record at gridDim.x + blockIdx.x; k_fused_arm: [6] the start time.
  __device__ __forceinline__ void store(long long *const stamps, const bool two) {
    if (threadIdx.x == 0) {
      long long *o = stamps + (size_t)blockIdx.x * 8;
      if (two) {
        long long *o2 = stamps + (size_t)(gridDim.x + blockIdx.x) * 8;
        for (int i = 0; i < 8; i++) o2[i] = sec[i];
      }
      for (int i = 0; i < 4; i++) o[i] = ph[i];
      o[4] = __builtin_amdgcn_s_memtime() - t_start;
      o[5] = (long long)pass | ((long long)both << 32);
      o[6] = two ? hand : t_start;
      o[7] = (long long)ipass | ((long long)nhand << 32);
    }
  }
};
#else
struct SecStamps {
  __device__ __forceinline__ void start() {}
  __device__ __forceinline__ void operator()(int) {}
  template <class O> __device__ __forceinline__ void put(O &, int, int) const {}
  template <class O> __device__ __forceinline__ void get(const O &, int, int) {}
  __device__ __forceinline__ void flush(bool, int) {}
};
struct PassStamps {
  __device__ __forceinline__ void start() {}
  __device__ __forceinline__ void hand_begin() {}
  __device__ __forceinline__ void hand_events(bool, bool) {}
  __device__ __forceinline__ void hand_end() {}
  __device__ __forceinline__ void pass_begin(bool, bool) {}
  __device__ __forceinline__ void mark() {}
  __device__ __forceinline__ void operator()(int) {}
  template <class O> __device__ __forceinline__ void sections(O) {}
  __device__ __forceinline__ void sweep_returned() {}
  __device__ __forceinline__ void sweep_reduced() {}
  __device__ __forceinline__ void sweep_end() {}
  __device__ __forceinline__ void store(long long *, bool) {}
};
#endif

// Order in which sweep_body takes the variables of a stage (positions 0 .. NV-1; the first NFIRST of them before
// the kinematics: see EARLY in sweep_body).
template <class C, bool EARLY>
struct SweepOrder {
  static constexpr int NFIRST = EARLY ? (C::NV - C::NQ - (C::NS > 0 ? 1 : 0)) : 0;
  __host__ __device__ static constexpr int at(int p) {
    int idx[C::NV] = {};
    int n = 0;
    if (EARLY) {
      for (int j = C::NQ; j < C::NV; j++)
        if (!(C::NS > 0 && j == C::NX)) idx[n++] = j;
      for (int j = 0; j < C::NQ; j++) idx[n++] = j;
      if (C::NS > 0) idx[n++] = C::NX;
    } else {
      for (int j = 0; j < C::NV; j++) idx[n++] = j;
    }
    return idx[p];
  }
};

// The scalars of the model the sweep needs (everything else comes through the view)
struct SweepK { int N; double dt; int use_curv; };

// FIRSTC: 1 / 0 = the first pass of a solve (or not) known at compile time, -1 = taken from first_rt.  The rows
// branch on it; callers that can afford two copies of the body (every kernel here) pass it as a constant so that
// the rows of a stage form one basic block and their requests are issued together.
// PHASE: 0 = the whole body.  1 / 2 = the merged form of the fused kernel, for passes that are not the first of a solve:
// 1 issues every request of the stage once -- what the body needs at its top and the slacks and multipliers of all the
// single-variable rows (top) -- and forms the step lengths of the stage from the loaded values (slen: what step_body
// computes, same rows in the same order); 2 continues from the registers of `top` with the step lengths the caller
// reduced over the stages in between, and requests none of tc, lc, gro, jqo, zc, dzp again.
template <class C, int EARLY_MODE = -1, class RP = gdouble, class V = RtView, int FIRSTC = -1, int PHASE = 0>
__device__ __forceinline__ void sweep_body(const SweepK M, const V &v, const SweepIO<RP> &io, const int k,
                                           const bool first_rt, const bool nostep, const double alpha, const double adual,
                                           const double mu, Partials &out, ldouble *const qacc = nullptr,
                                           SweepTop<C, V> *const top = nullptr, StepRow<C> *const slen = nullptr) {
  static_assert(PHASE == 0 || (FIRSTC == 0 && V::SPEC), "the merged form: static rows, not the first pass of a solve");
  const bool first = FIRSTC < 0 ? first_rt : (FIRSTC != 0);
  // (FKCURV, k_sweep) the two 7 x 7 blocks of the q variables are accumulated in LDS, one column of 2 x 28 doubles per
  // lane (qacc, lane stride kSweepBlock): they are touched once per FK point and by the joint-limit rows only, and the
  // kernel has no register to spare for them
  constexpr bool QLDS = C::FKCURV;
  auto qtri = [](int a, int c) __attribute__((always_inline)) { return a * C::NQ - a * (a - 1) / 2 + (c - a); };
  SecStamps st;
  st.start();
  constexpr int NQ = C::NQ, NX = C::NX, NS = C::NS, NU = C::NU, NV = C::NV;
  const int N = M.N;
  const unsigned loff = io.loff;
  const size_t SS = io.SS;
  const gdouble *__restrict__ zc = io.zc;
  const gdouble *__restrict__ tc = io.tc;
  const gdouble *__restrict__ lc = io.lc;
  const gdouble *__restrict__ nc = io.nc;
  gdouble *__restrict__ zn = io.zn;
  gdouble *__restrict__ tn = io.tn;
  gdouble *__restrict__ ln = io.ln;
  gdouble *__restrict__ nn = io.nn;
  const gdouble *__restrict__ pp = io.pp;
  const RP *__restrict__ dzp = io.dzp;
  const gdouble *__restrict__ gro = io.gro;   // row values and FK-row gradients at the current iterate:
  const gdouble *__restrict__ jqo = io.jqo;   //  the slack / multiplier steps are recomputed from them
  gdouble *__restrict__ grn = io.grn;
  gdouble *__restrict__ jqn = io.jqn;
  const RP *__restrict__ nup = io.nup;
  gdouble *__restrict__ gfa = io.gfa;
  RP *__restrict__ rec = (RP *)__builtin_assume_aligned(io.rec, 64);   // 64-byte aligned: neighbouring entries leave as 16-byte stores

  // ---- trial stage vector, costates, next stage's state ------------------------
  double z[NV], xk1[NX], nuk[NX], nun[NX];
  SweepTop<C, V> top_local;
  SweepTop<C, V> &T = PHASE == 0 ? top_local : *top;
  auto &zo = T.zo; auto &dzo = T.dzo;
  const unsigned loff1 = loff + (k < N - 1 ? io.kstride : 0u);  // next stage, clamped: loads stay unconditional
  const bool warm = first && (io.warm != 0);
  // multipliers the rows start from: the current buffer, or (warm first pass) the previous solve's, one stage on
  const gdouble *__restrict__ lsrc = warm ? io.wl : lc;
  const unsigned loffl = warm ? loff1 : loff;
#define IDXLL(slot) ((size_t)(slot) * SS + loffl)
  auto &x1 = T.x1; auto &dx1 = T.dx1; auto &n0 = T.n0; auto &n0n = T.n0n; auto &n1 = T.n1; auto &n1n = T.n1n;
  if constexpr (PHASE != 2) {
    const size_t SSd = io.SSd;
    const unsigned loffd = io.loffd, loffd1 = io.loffd + (k < N - 1 ? io.kstrided : 0u);
#pragma unroll
    for (int j = 0; j < NV; j++) { zo[j] = zc[IDXL(j)]; dzo[j] = dzp[(size_t)j * SSd + loffd]; }
#pragma unroll
    for (int j = 0; j < NX; j++) {
      x1[j] = zc[IDXL1(j)]; dx1[j] = dzp[(size_t)j * SSd + loffd1];
      n0[j] = nc[IDXL(j)];  n0n[j] = nup[(size_t)j * SSd + loffd];
      n1[j] = nc[IDXL1(j)]; n1n[j] = nup[(size_t)j * SSd + loffd1];
    }
  }
  auto P = [&](int off) __attribute__((always_inline)) -> double { return pp[IDXL(off)]; };
  // Request batching (generated views: PIPE).  One wavefront per SIMD hides no latency by itself, so the body issues
  // what it will need well before it needs it: the objective parameters and every distance row's inputs here, the
  // single-variable rows two variables ahead of the arithmetic (var_load / var_compute below).  With the runtime
  // tables the requests stay where the arithmetic is, as before.
  // (the arms too, over the runtime tables: their sweep waits on memory for 63 % of its cycles -- 114 -> 110 us)
  constexpr bool PIPE = V::SPEC || C::FKCURV || std::is_same<V, GView>::value;
  auto &wuv = T.wuv; auto &wsv = T.wsv; auto &goalv = T.goalv; auto &wgoalv = T.wgoalv;
  if constexpr (PHASE != 2) {
    wsv = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) { goalv[c] = 0.0; wgoalv[c] = 0.0; }
#pragma unroll
    for (int j = 0; j < NU; j++) wuv[j] = P(v.off_wu() + j);
    if constexpr (NS > 0) wsv = P(v.off_ws());
    T.rbody = (v.off_r_body() >= 0) ? P(v.off_r_body()) : 0.0;
    if (v.has_goal()) {
#pragma unroll
      for (int c = 0; c < 3; c++) { goalv[c] = P(v.off_goal() + c); wgoalv[c] = P(v.off_wgoal() + c); }
    }
  }
  const double rbody = T.rbody;
  using FkBuf = SweepFkBuf<NQ>;
  auto fk_load = [&](const int r, FkBuf &Bf) __attribute__((always_inline)) {
    const int i = v.fk_row(r), kind = v.fk_kind(r), ob = v.fk_obst(r), fi = v.fk_idx(r);
    Bf.tcv = tc[IDXL(i)]; Bf.lcv = lsrc[IDXLL(i)]; Bf.gold = gro[IDXL(i)];
#pragma unroll
    for (int a = 0; a < NQ; a++) Bf.jo[a] = jqo[IDXL(fi * NQ + a)];
#pragma unroll
    for (int c = 0; c < 4; c++) Bf.op[c] = 0.0;
    if (kind == ROW_RADIAL) {
#pragma unroll
      for (int c = 0; c < 4; c++) Bf.op[c] = P(v.off_obst() + 4 * ob + c);
    } else if (kind == ROW_LINEAR) {
#pragma unroll
      for (int c = 0; c < 4; c++) Bf.op[c] = P(v.off_lin() + 4 * ob + c);
    }
    Bf.wi = 0.0;
    if (v.has_avoid() && v.fk_first(r)) Bf.wi = P(v.off_wconstr() + v.fk_mod(r));
  };
  constexpr int NFKC = SweepTop<C, V>::NFKC;
  auto &fkb = T.fkb;
  if constexpr (V::SPEC && PHASE != 2) {   // (the rows of a generated view are static: their inputs are requested here, all at once)
    for_range<0, NFKC>([&](auto rc) __attribute__((always_inline)) {
      constexpr int r = decltype(rc)::value;
      if constexpr (r < V::nfkrows()) fk_load(r, fkb[r]);
    });
  }

  struct VarBuf { double tcv[kVarRows], lcv[kVarRows], lim[kVarRows], wi[kVarRows]; };
  auto var_load = [&](auto jc, VarBuf &Bv) __attribute__((always_inline)) {
    constexpr int j = decltype(jc)::value;
    // unconditional, clamped requests for the (up to) four rows of variable j
#pragma unroll
    for (int u = 0; u < kVarRows; u++) {
      const int i = v.v_row(j, u);
      const int ii = i >= 0 ? i : 0;
      const int po = v.v_poff(j, u);
      if constexpr (PHASE == 0) {   // (merged form: requested once, at the top of the call -- T.vt / T.vl)
        Bv.tcv[u] = tc[IDXL(ii)];
        Bv.lcv[u] = lsrc[IDXLL(ii)];
      }
      const double pl = pp[IDXL(po >= 0 ? po : 0)];
      Bv.lim[u] = po >= 0 ? pl : v.v_val(j, u);
      Bv.wi[u] = 0.0;
      if (i >= 0 && v.has_avoid() && v.v_first(j, u)) Bv.wi[u] = P(v.off_wconstr() + v.v_mod(j, u));
    }
  };
  if constexpr (PHASE == 1) {
    // ---- merged form: the rest of the stage's requests, then the step lengths from the loaded values -------------
    // (what step_body does, on the words the sweep holds anyway; only the cost gradient and the stored values of the
    //  general rows are requested for the step lengths alone)
    double gfv[NV], gl[NV][kVarRows];
#pragma unroll
    for (int j = 0; j < NV; j++) {
      gfv[j] = gfa[IDXL(j)];
#pragma unroll
      for (int u = 0; u < kVarRows; u++) {
        const int i = v.v_row(j, u);
        gl[j][u] = 0.0;
        if (i < 0) continue;   // (static rows)
        T.vt[j][u] = tc[IDXL(i)];
        T.vl[j][u] = lc[IDXL(i)];
        if (v.v_poff(j, u) >= 0) gl[j][u] = gro[IDXL(i)];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    StepRow<C> &sr = *slen;
    sr.slope(gfv, dzo);
    for_range<0, V::nfkrows()>([&](auto rc) __attribute__((always_inline)) {
      constexpr int r = decltype(rc)::value;
      sr.template fk_row<V>(mu, dzo, fkb[r].gold, fkb[r].tcv, fkb[r].lcv, fkb[r].jo);
    });
#pragma unroll
    for (int j = 0; j < NV; j++) {
#pragma unroll
      for (int u = 0; u < kVarRows; u++) {
        if (v.v_row(j, u) < 0) continue;
        sr.template var_row<V>(v, k, mu, j, u, zo, dzo, gl[j][u], T.vt[j][u], T.vl[j][u]);
      }
    }
    return;
  }
  const double al = alpha, adl = adual;
  // ---- trial point -----------------------------------------------------------------------------------
  {
#pragma unroll
    for (int j = 0; j < NV; j++) {
      z[j] = nostep ? zo[j] : zo[j] + al * dzo[j];
      zn[IDXL(j)] = z[j];
    }
#pragma unroll
    for (int j = 0; j < NX; j++) {
      xk1[j] = nostep ? x1[j] : x1[j] + al * dx1[j];
      if constexpr (QLDS) qacc[(2 * C::NQ2 + j) * kSweepBlock] = xk1[j];   // (read back for the defect, at the end)
      double v = 0.0, w = 0.0;
      if (!first && k >= 1) v = nostep ? n0[j] : n0[j] + al * (n0n[j] - n0[j]);
      if (!first && k < N - 1) w = nostep ? n1[j] : n1[j] + al * (n1n[j] - n1[j]);
      if (warm) {
        // costates of the previous solve, shifted: nu_k <- nu_{k+1}, nu_{k+1} <- nu_{k+2} (last stage repeated)
        const unsigned loff2 = loff1 + (k < N - 2 ? io.kstride : 0u);
        if (k >= 1) v = io.wn[IDXL1(j)];
        if (k < N - 1) w = io.wn[(size_t)j * SS + loff2];
      }
      nuk[j] = v;
      if constexpr (QLDS) { if (j < NQ) qacc[(2 * C::NQ2 + NX + (j < NQ ? j : 0)) * kSweepBlock] = v; }
      nun[j] = w;
      nn[IDXL(j)] = v;
    }
  }
  // ---- accumulators --------------------------------------------------------
  double gf[NV], q0[NV], q1[NV], rs[NV], Dg[NV], cs[NV];
  double Qqq[NQ][NQ];
  constexpr bool QC = C::CURV || C::DDCURV;   // the record carries a curvature block of the q variables
  double Cqq[QC ? NQ : 1][QC ? NQ : 1];  // sum_i (lambda_i + cN/h^2) grad^2 h_i of the distance rows
#pragma unroll
  for (int a = 0; a < (QC ? NQ : 1); a++)
#pragma unroll
    for (int c = 0; c < (QC ? NQ : 1); c++) Cqq[a][c] = 0;
#pragma unroll
  for (int j = 0; j < NV; j++) { gf[j] = 0; q0[j] = 0; q1[j] = 0; rs[j] = 0; Dg[j] = 0; cs[j] = 0; }
#pragma unroll
  for (int a = 0; a < NQ; a++)
#pragma unroll
    for (int c = 0; c < NQ; c++) Qqq[a][c] = 0;
  if constexpr (QLDS) {
#pragma unroll
    for (int s2 = 0; s2 < 2 * C::NQ2; s2++) qacc[s2 * kSweepBlock] = 0.0;
  }
  double f = 0.0;
  int bad = 0;
  double theta = 0.0, rineq = 0.0, rcomp = 0.0, sumc = 0.0, minc = 1e300;
  // sum of log t over the rows, kept as log(prod of mantissas) + ln2 * (sum of exponents): one log per lane
  // instead of one per row (a software log is ~70 instructions; the rows of a stage are the bulk of this kernel)
  double lprod = 1.0;
  int lexp = 0;

  st(0);
  // ---- control effort and slack penalty (ObjectiveManager.py:28-42) ----------
#pragma unroll
  for (int j = 0; j < NU; j++) {
    const double wu = wuv[j], u = z[NX + NS + j];
    f += wu * u * u;
    gf[NX + NS + j] += 2.0 * wu * u;
    Dg[NX + NS + j] += 2.0 * wu;
  }
  double sl = 0.0;
  if constexpr (NS > 0) {
    const double ws = wsv;
    sl = z[NX];
    f += ws * sl * sl;
    gf[NX] += 2.0 * ws * sl;
    Dg[NX] += 2.0 * ws;
  }
  // trial slack / multiplier of row i and their bookkeeping; returns sigma, ca, cb, lv
  struct RowW { double sig, ca, cb, lv; };
  // (gold, gdz: row value at the current iterate and J_i dz -- the slack / multiplier steps of the row are
  //  recomputed with the very expressions k_step took its step lengths from)
  auto row_core = [&](int i, double g, double tcv, double lcv, double gold, double gdz) __attribute__((always_inline)) -> RowW {
    double tv, lv;
    if (first) {
      const double tmin = warm ? kWarmTMin : kTMin;
      tv = g > tmin ? g : tmin;
      lv = mu * frcp(tv);
      if (warm) lv = lcv > lv ? lcv : lv;   // (lcv: the previous solve's multiplier of this row, one stage on)
    } else {
      const double dtv = gdz + (gold - tcv);
      const double dlv = (mu - tcv * lcv - lcv * dtv) * frcp(tcv);
      // (null passes keep the point by selection, not by a zero step length: the step they would multiply
      //  may be stale -- after a failed factorisation of the fused kernel even non-finite)
      tv = nostep ? tcv : tcv + al * dtv;
      lv = nostep ? lcv : lcv + adl * dlv;
    }
    tn[IDXL(i)] = tv;
    ln[IDXL(i)] = lv;
    const double rg = g - tv;
    theta += fabs(rg);
    bad |= (int)!(tv > 0.0);   // (cannot happen: fraction to the boundary; keeps the product's sign meaningful.  |=: no branch)
    {
      int ex;
      lprod *= frexp(tv, &ex);
      lexp += ex;
    }
    rineq = fmax(rineq, fabs(rg));
    const double cmp = tv * lv;
    rcomp = fmax(rcomp, cmp);
    sumc += cmp;
    minc = fmin(minc, cmp);
    const double it = frcp(tv);
    return {lv * it, lv * rg * it, it, lv};
  };

  // ---- single-variable rows: limits (general rows) and simple bounds, by variable ----
  // (generic lambda over a compile-time variable index: every array index stays a constant)
  auto var_compute = [&](auto jc, const VarBuf &Bv) __attribute__((always_inline)) {
    constexpr int j = decltype(jc)::value;
#pragma unroll
    for (int u = 0; u < kVarRows; u++) {
      const int i = v.v_row(j, u);
      if (i < 0) continue;  // uniform
      const double sg = (double)v.v_sgn(j, u);
      const bool soft = (NS > 0) && v.v_soft(j, u);
      const bool neutral = (k == 0) && (j < NX) && !soft;  // constant of the problem at the pinned stage
      const double h = neutral ? 1.0 : sg * (z[j] - Bv.lim[u]);
      if (v.has_avoid() && v.v_first(j, u)) {
        // (selects, not a branch on the weight: a data-dependent branch would cut the stage's rows into
        //  separate basic blocks and with them the batches of requests)
        const double wi = Bv.wi[u];
        const bool on = (wi != 0.0) && !(k == 0 && j < NX);
        const double cN = (double)M.N * wi;
        bad |= (int)(on & !(h > 0.0));   // (bitwise: a short-circuit branch would cut the rows into separate basic blocks)
        const double ih = frcp(h);
        f += on ? cN * ih : 0.0;
        gf[j] += on ? -cN * (ih * ih) * sg : 0.0;
        const double c2 = on ? 2.0 * cN * (ih * ih * ih) : 0.0;
        if (j < NQ) {
          if constexpr (QLDS) qacc[qtri(j < NQ ? j : 0, j < NQ ? j : 0) * kSweepBlock] += c2;
          else Qqq[j < NQ ? j : 0][j < NQ ? j : 0] += c2;
        } else Dg[j] += c2;
      }
      double g = h;
      if constexpr (NS > 0) { if (soft) g += sl; }
      if (v.v_poff(j, u) >= 0) grn[IDXL(i)] = g;  // general rows keep their value for k_step
      // the same row at the current iterate (what k_step read back or recomputed)
      double gold = neutral ? 1.0 : sg * (zo[j] - Bv.lim[u]);
      double gdz = sg * dzo[j];
      if constexpr (NS > 0) { if (soft) { gold += zo[NX]; gdz += dzo[NX]; } }
      double tcv, lcv;
      if constexpr (PHASE == 0) { tcv = Bv.tcv[u]; lcv = Bv.lcv[u]; }
      else { tcv = T.vt[j][u]; lcv = T.vl[j][u]; }
      const RowW rw = row_core(i, g, tcv, lcv, gold, gdz);
      // (a neutralised row contributes nothing; by selection, not by a branch: in the fused kernel the stage differs
      //  from lane to lane and a divergent `continue` cuts the rows of a variable into exec-masked blocks)
      q0[j] = neutral ? q0[j] : q0[j] + sg * rw.ca;
      q1[j] = neutral ? q1[j] : q1[j] + sg * rw.cb;
      rs[j] = neutral ? rs[j] : rs[j] - sg * rw.lv;
      const double sigc = neutral ? 0.0 : rw.sig;
      if (j < NQ) {
        if constexpr (QLDS) qacc[qtri(j < NQ ? j : 0, j < NQ ? j : 0) * kSweepBlock] += sigc;
        else Qqq[j < NQ ? j : 0][j < NQ ? j : 0] = neutral ? Qqq[j < NQ ? j : 0][j < NQ ? j : 0] : Qqq[j < NQ ? j : 0][j < NQ ? j : 0] + rw.sig;
      } else Dg[j] = neutral ? Dg[j] : Dg[j] + rw.sig;
      if constexpr (NS > 0) {
        if (soft) {
          cs[j] += rw.sig * sg;
          q0[NX] += rw.ca;
          q1[NX] += rw.cb;
          rs[NX] -= rw.lv;
          Dg[NX] += rw.sig;
        }
      }
    }
  };
  // Everything variable j contributes to is complete: stationarity residual of the variable and its entries
  // of the stage record.  (Holonomic chain: A^T nu = [nu_q ; dt nu_q + nu_v], B^T nu = dt^2/2 nu_q + dt nu_v;
  // the diff-drive model needs its Jacobians first and is finalised in one go further down.)
  double rstat = 0.0;
  auto finalize_var = [&](auto jc) __attribute__((always_inline)) {
    constexpr int j = decltype(jc)::value;
    double r = rs[j] + gf[j];
    if constexpr (C::ROBOT == RMPC_ROBOT_CHAIN) {
      if (k < N - 1) {
        const double hh = M.dt, hh2 = 0.5 * M.dt * M.dt;
        if constexpr (j < NQ) r += nun[j];
        else if constexpr (j < NX) r += hh * nun[j - NQ] + nun[j];
        else if constexpr (j >= NX + NS) r += hh2 * nun[j - NX - NS] + hh * nun[NQ + (j - NX - NS)];
      }
    }
    if (!(j < NX && k == 0)) {   // x_1 is fixed: no stationarity condition
      if constexpr (j < NX) {
        if constexpr (QLDS && j < NQ) r -= qacc[(2 * C::NQ2 + NX + j) * kSweepBlock];
        else r -= nuk[j];
      }
      rstat = fmax(rstat, fabs(r));
    }
    if constexpr (j >= NQ) rec[C::R_DG + j - NQ] = Dg[j];
    if constexpr (NS > 0) rec[C::R_CS + j] = cs[j];
    rec[C::R_Q0 + j] = gf[j] + q0[j];
    rec[C::R_Q1 + j] = q1[j];
    gfa[IDXL(j)] = gf[j];
  };
  constexpr bool CHAIN = (C::ROBOT == RMPC_ROBOT_CHAIN);
  // The arm: velocity and input variables first, so that their accumulators are dead before the kinematics
  // start (the slack variable collects from every softened row and waits for the end): 1.2 KB less scratch
  // per lane, sweep 190 -> 139 us on cfg4.  The three-joint models do not spill and lose 7 % this way.
  constexpr bool EARLY = (EARLY_MODE >= 0) ? (CHAIN && EARLY_MODE != 0) : (CHAIN && (NQ > 3));
  using Ord = SweepOrder<C, EARLY>;
  // positions [P0, P1) of the order; PIPE: the requests of a variable are issued two variables ahead (the first two
  // of the range by the caller when PRE is set)
  // (PD: how many variables ahead.  Two: the boxer over the runtime tables at three and four -- a round trip to the
  //  instance's block is 2 - 3 us with the chip full, the rows of a variable 0.5 us -- spills 428 / 556 B per lane instead
  //  of 296 and loses 4 - 7 %: 0.68 -> 0.64 M solves/s with four batches in flight)
  constexpr int PD = 2;
  VarBuf vring[PIPE ? PD + 1 : 1];
  auto run_vars = [&](auto p0c, auto p1c, auto finc, auto prec) __attribute__((always_inline)) {
    constexpr int P0 = decltype(p0c)::value, P1 = decltype(p1c)::value;
    constexpr bool FIN = decltype(finc)::value, PRE = decltype(prec)::value;
    if constexpr (P1 > P0) {
      if constexpr (PIPE && !PRE) {
        for_range<0, PD>([&](auto dc) __attribute__((always_inline)) {
          constexpr int d = decltype(dc)::value;
          if constexpr (P0 + d < P1) var_load(std::integral_constant<int, Ord::at(P0 + d < P1 ? P0 + d : P0)>{}, vring[d]);
        });
      }
      for_range<P0, P1>([&](auto pc) __attribute__((always_inline)) {
        constexpr int p = decltype(pc)::value;
        constexpr int j = Ord::at(p);
        if constexpr (PIPE) {
          if constexpr (p + PD < P1) var_load(std::integral_constant<int, Ord::at(p + PD < P1 ? p + PD : p)>{}, vring[(p + PD - P0) % (PD + 1)]);
          __builtin_amdgcn_sched_barrier(0);
          var_compute(std::integral_constant<int, j>{}, vring[(p - P0) % (PD + 1)]);
        } else {
          var_load(std::integral_constant<int, j>{}, vring[0]);
          var_compute(std::integral_constant<int, j>{}, vring[0]);
        }
        if constexpr (FIN) finalize_var(std::integral_constant<int, j>{});
      });
    }
  };
  using TrueT = std::integral_constant<bool, true>;
  using FalseT = std::integral_constant<bool, false>;
  run_vars(std::integral_constant<int, 0>{}, std::integral_constant<int, Ord::NFIRST>{}, TrueT{}, FalseT{});
  // (no variable goes first: the requests of the first PD variables leave before the kinematics)
  constexpr bool PRE2 = PIPE && (Ord::NFIRST == 0);
  if constexpr (PRE2) {
    for_range<0, PD>([&](auto dc) __attribute__((always_inline)) {
      constexpr int d = decltype(dc)::value;
      if constexpr (d < NV) var_load(std::integral_constant<int, Ord::at(d < NV ? d : 0)>{}, vring[d]);
    });
  }

  // ---- kinematics, GoalReaching and the FK rows, slot by slot -------------------
  Kin<C> kin;
  {
    double q[NQ];
#pragma unroll
    for (int j = 0; j < NQ; j++) q[j] = z[j];
    kin.compute(v, q);
  }
  auto do_slot = [&](auto slc) __attribute__((always_inline)) {
    constexpr int SL = decltype(slc)::value;
    if constexpr (V::SPEC) {
      if constexpr (SL >= V::nslots()) return;
    }
    if (SL >= v.nslots()) return;
    Vec3 J[NQ];
    const Vec3 Pt = kin.template point<SL>(v, J);
    // (DDCURV) the frames ride on the base, p = (x, y) + R(theta) o: d2 p / dtheta2 = -(p - (x, y)); a pair: -(pa - pb)
    Vec3 ddP = {0, 0, 0};
    if constexpr (C::DDCURV) {
      if (v.slot_fb(SL) >= 0) ddP = {-Pt.x, -Pt.y, 0.0};
      else ddP = {-(kin.pa[SL].x - kin.qx), -(kin.pa[SL].y - kin.qy), 0.0};
    }
    // (FKCURV) sum over the slot's rows of (multiplier + inverse-barrier weight) x unit direction of the row, minus
    // the goal cost's 2 w e: what the second derivatives of the slot's point are contracted with
    Vec3 Fc = {0, 0, 0};
    // (FKCURV) every term a row of the slot adds to the q block has the form J^T (w n n^T) J with the row's unit
    // direction n in the slot's point: the rows accumulate 3 x 3 symmetric matrices (xx xy xz yy yz zz) and the
    // 7 x 7 blocks are formed once per slot -- 6 multiply-adds per row instead of 28, and the 2 x 28 block entries
    // are not read-modify-written inside the row loop (the arm's sweep lives in scratch: 1276 -> 1140 bytes per lane, 126 -> 115 us)
    double TQ[6] = {0, 0, 0, 0, 0, 0}, TC[6] = {0, 0, 0, 0, 0, 0};
    double Wsum = 0.0;
    auto addsym = [](double (&T)[6], const double w, const Vec3 &n) __attribute__((always_inline)) {
      const double wx = w * n.x, wy = w * n.y, wz = w * n.z;
      T[0] += wx * n.x; T[1] += wx * n.y; T[2] += wx * n.z; T[3] += wy * n.y; T[4] += wy * n.z; T[5] += wz * n.z;
    };
    if (SL == 0 && v.has_goal()) {
      // GoalReaching (goal_reaching.py:19-33), Gauss-Newton Hessian
      const double e0 = Pt.x - goalv[0], e1 = Pt.y - goalv[1], e2 = Pt.z - goalv[2];
      const double w0 = wgoalv[0], w1 = wgoalv[1], w2 = wgoalv[2];
      f += w0 * e0 * e0 + w1 * e1 * e1 + w2 * e2 * e2;
#pragma unroll
      for (int a = 0; a < NQ; a++) {
        gf[a] += 2.0 * (w0 * e0 * J[a].x + w1 * e1 * J[a].y + w2 * e2 * J[a].z);
        if constexpr (!C::FKCURV) {
#pragma unroll
          for (int c = a; c < NQ; c++)
            Qqq[a][c] += 2.0 * (w0 * J[a].x * J[c].x + w1 * J[a].y * J[c].y + w2 * J[a].z * J[c].z);
        }
      }
      if constexpr (C::FKCURV) {
        TQ[0] += 2.0 * w0; TQ[3] += 2.0 * w1; TQ[5] += 2.0 * w2;
        Fc = {-2.0 * w0 * e0, -2.0 * w1 * e1, -2.0 * w2 * e2};
      }
      if constexpr (C::DDCURV) {
        // what Gauss-Newton leaves out: 2 sum_c w_c e_c d2 p_c / dtheta2 (added to Q: subtracted from the block that is subtracted)
        Cqq[2][2] -= 2.0 * (w0 * e0 * ddP.x + w1 * e1 * ddP.y);
      }
    }
    auto fk_row_body = [&](const int r, const FkBuf &Bf) __attribute__((always_inline)) {
      const int i = v.fk_row(r), kind = v.fk_kind(r);
      const int fi = v.fk_idx(r);
      const double tcv = Bf.tcv, lcv = Bf.lcv, gold = Bf.gold;
      double gdz = 0.0;
      {
#pragma unroll
        for (int a = 0; a < NQ; a++) gdz += Bf.jo[a] * dzo[a];
        if constexpr (NS > 0) gdz += dzo[NX];
      }
      double gq[NQ];
      double h, cinv = 0.0;
      double ndd = 0.0;      // unit direction of the row . d2 p / dtheta2 (DDCURV)
      Vec3 nd = {0, 0, 0};   // unit direction of the row in the slot's point (FKCURV)
      if (kind == ROW_RADIAL) {
        // ||fk_l(q) - c_i|| - r_i - r_body (mpcBase.py:82-101)
        const Vec3 dv = {Pt.x - Bf.op[0], Pt.y - Bf.op[1], Pt.z - Bf.op[2]};
        const double dist = sqrt(dot(dv, dv));
        h = dist - Bf.op[3] - rbody;
        cinv = 1.0 / dist;
        if constexpr (C::FKCURV) nd = {dv.x * cinv, dv.y * cinv, dv.z * cinv};
        if constexpr (C::DDCURV) ndd = dot(dv, ddP) * cinv;
#pragma unroll
        for (int a = 0; a < NQ; a++) gq[a] = dot(dv, J[a]) * cinv;
      } else if (kind == ROW_LINEAR) {
        // |a.fk_l(q) + d| / ||a|| - r_body (LinearConstraints.py:25-40, utils.py:48-52)
        const Vec3 av = {Bf.op[0], Bf.op[1], Bf.op[2]};
        const double nrm = sqrt(dot(av, av));
        const double sd = dot(av, Pt) + Bf.op[3];
        const double sgn = sd < 0 ? -1.0 : 1.0;
        h = fabs(sd) / nrm - rbody;
        if constexpr (C::FKCURV) nd = {sgn * av.x / nrm, sgn * av.y / nrm, sgn * av.z / nrm};
        if constexpr (C::DDCURV) ndd = sgn * dot(av, ddP) / nrm;
#pragma unroll
        for (int a = 0; a < NQ; a++) gq[a] = sgn * dot(av, J[a]) / nrm;
      } else {
        // ||fk_a(q) - fk_b(q)|| - 2 r_body (SelfCollisionAvoidanceConstraints.py:19-27)
        const double dist = sqrt(dot(Pt, Pt));
        h = dist - 2.0 * rbody;
        cinv = 1.0 / dist;
        if constexpr (C::FKCURV) nd = {Pt.x * cinv, Pt.y * cinv, Pt.z * cinv};
        if constexpr (C::DDCURV) ndd = dot(Pt, ddP) * cinv;
#pragma unroll
        for (int a = 0; a < NQ; a++) gq[a] = dot(Pt, J[a]) * cinv;
      }
      // stage 1 (state pinned to xinit): state-only, unsoftened rows are constants of the
      // problem -- neutralised (value 1, zero gradient, no inverse-barrier term); DESIGN.md 2
      if (k == 0 && NS == 0) {
        h = 1.0;
        cinv = 0.0;
        ndd = 0.0;
        nd = {0, 0, 0};
#pragma unroll
        for (int a = 0; a < NQ; a++) gq[a] = 0.0;
      }
      double cw = 0.0, c2row = 0.0;
      if (v.has_avoid() && v.fk_first(r)) {
        // inverse-barrier objective N w_i / h on the first row of a module (constraint_avoidance.py:22-31)
        const double wi = Bf.wi;
        const bool on = (wi != 0.0) && (k != 0);   // (selects: see the single-variable rows)
        const double cN = (double)M.N * wi;
        bad |= (int)(on & !(h > 0.0));   // (bitwise: a short-circuit branch would cut the rows into separate basic blocks)
        const double ih = frcp(h);
        f += on ? cN * ih : 0.0;
        const double c1 = on ? -cN * (ih * ih) : 0.0, c2 = on ? 2.0 * cN * (ih * ih * ih) : 0.0;
        cw = on ? cN * (ih * ih) : 0.0;
        c2row = c2;
#pragma unroll
        for (int a = 0; a < NQ; a++) {
          gf[a] += c1 * gq[a];
          if constexpr (!C::FKCURV) {
#pragma unroll
            for (int c = a; c < NQ; c++) Qqq[a][c] += c2 * gq[a] * gq[c];
          }
        }
      }
      double g = h;
      if constexpr (NS > 0) g += sl;  // softened rows (intended InequalityManager.py:29-32)
      grn[IDXL(i)] = g;
#pragma unroll
      for (int a = 0; a < NQ; a++) jqn[IDXL(fi * NQ + a)] = gq[a];
      const RowW rw = row_core(i, g, tcv, lcv, gold, gdz);
#pragma unroll
      for (int a = 0; a < NQ; a++) {
        q0[a] += gq[a] * rw.ca;
        q1[a] += gq[a] * rw.cb;
        rs[a] -= gq[a] * rw.lv;
        if constexpr (!C::FKCURV) {
#pragma unroll
          for (int c = a; c < NQ; c++) Qqq[a][c] += rw.sig * gq[a] * gq[c];
        }
        if constexpr (NS > 0) cs[a] += rw.sig * gq[a];
      }
      if constexpr (C::FKCURV) addsym(TQ, rw.sig + c2row, nd);
      if constexpr (NS > 0) {
        q0[NX] += rw.ca;
        q1[NX] += rw.cb;
        rs[NX] -= rw.lv;
        Dg[NX] += rw.sig;
      }
      if constexpr (QC) {
        // exact Hessian of the distance rows when the kinematics are affine in q:
        // grad^2 h = (J^T J - g g^T) / dist, weighted by the multiplier and the inverse-barrier term
        // (weight selected, not branched on: the rows of the slot stay one basic block)
        const double wgt = (M.use_curv && kind != ROW_LINEAR) ? (rw.lv + cw) * cinv : 0.0;
        if constexpr (C::FKCURV) {
          // (J^T J - g g^T) / dist = J^T (I - n n^T) J / dist
          Wsum += wgt;
          addsym(TC, wgt, nd);
          const double wf = rw.lv + cw;
          Fc.x += wf * nd.x; Fc.y += wf * nd.y; Fc.z += wf * nd.z;
        } else {
#pragma unroll
          for (int a = 0; a < NQ; a++)
#pragma unroll
            for (int c = a; c < NQ; c++) Cqq[a][c] += wgt * (dot(J[a], J[c]) - gq[a] * gq[c]);
          // (the unicycle: the frame turns with the base -- the row's direction times d2 p / dtheta2)
          if constexpr (C::DDCURV) Cqq[2][2] += M.use_curv ? (rw.lv + cw) * ndd : 0.0;
        }
      }
    };
    if constexpr (V::SPEC) {
      // generated view: the rows of the slot are known at compile time -- straight-line code
      for_range<0, V::nfkrows()>([&](auto rc) __attribute__((always_inline)) {
        constexpr int r = decltype(rc)::value;
        if constexpr (r >= V::slot_row_begin(SL) && r < V::slot_row_begin(SL + 1)) fk_row_body(r, fkb[r]);
      });
    } else {
      // (runtime tables: the requests of the next row of the slot leave before this row's arithmetic)
      const int rb0 = v.slot_row_begin(SL), re0 = v.slot_row_begin(SL + 1);
      if constexpr (C::FKCURV) {
        // (the arms: no register to spare for a second row's inputs -- 420 -> 564 B of scratch, sweep 98 -> 102 us)
        for (int r = rb0; r < re0; r++) {
          fk_load(r, fkb[0]);   // requests first, arithmetic after
          fk_row_body(r, fkb[0]);
        }
      } else if (rb0 < re0) {
        FkBuf nxt;
        fk_load(rb0, nxt);
        for (int r = rb0; r < re0; r++) {
          fkb[0] = nxt;
          fk_load(r + 1 < re0 ? r + 1 : r, nxt);
          __builtin_amdgcn_sched_barrier(0);
          fk_row_body(r, fkb[0]);
        }
      }
    }
    if constexpr (C::FKCURV) {
      // second derivatives of the slot's point: for joints a before c on the chain dJ_c/dq_a = axis_a x J_c when
      // joint a is revolute (it turns everything behind it, the column J_c included), 0 when it is prismatic;
      // Fc . (axis_a x J_c) = (Fc x axis_a) . J_c.  Columns beyond the slot's frames are zero.
      auto symv = [](const double (&T)[6], const Vec3 &x) __attribute__((always_inline)) -> Vec3 {
        return {T[0] * x.x + T[1] * x.y + T[2] * x.z, T[1] * x.x + T[3] * x.y + T[4] * x.z, T[2] * x.x + T[4] * x.y + T[5] * x.z};
      };
#pragma unroll
      for (int a = 0; a < NQ; a++) {
        const Vec3 u = symv(TQ, J[a]);
#pragma unroll
        for (int c = a; c < NQ; c++) qacc[qtri(a, c) * kSweepBlock] += dot(u, J[c]);
      }
      if (M.use_curv) {
#pragma unroll
        for (int a = 0; a < NQ; a++) {
          const Vec3 t = symv(TC, J[a]);
          Vec3 w = {Wsum * J[a].x - t.x, Wsum * J[a].y - t.y, Wsum * J[a].z - t.z};
          if (v.joint_type(a) == RMPC_JOINT_REVOLUTE) {
            const Vec3 G = cross(Fc, kin.aj[a]);
            w = {w.x + G.x, w.y + G.y, w.z + G.z};
          }
#pragma unroll
          for (int c = a; c < NQ; c++) qacc[(C::NQ2 + qtri(a, c)) * kSweepBlock] += dot(w, J[c]);
        }
      }
    }
  };
  do_slot(std::integral_constant<int, 0>{});
  do_slot(std::integral_constant<int, 1>{});
  do_slot(std::integral_constant<int, 2>{});
  do_slot(std::integral_constant<int, 3>{});

  st(1);
  // ---- the remaining single-variable rows -----------------------------------------------
  run_vars(std::integral_constant<int, Ord::NFIRST>{}, std::integral_constant<int, NV>{}, FalseT{},
           std::integral_constant<bool, PRE2>{});

  st(2);
  // ---- dynamics defect and stationarity -------------------------------------------
  double req = 0.0;
  if constexpr (CHAIN) {
    if (k < N - 1) {
      double xn[NX];
      chain_step<C>(M.dt, z, xn);
#pragma unroll
      for (int j = 0; j < NX; j++) {
        const double r = xn[j] - (QLDS ? (double)qacc[(2 * C::NQ2 + j) * kSweepBlock] : xk1[j]);
        rec[C::R_RC + j] = r;
        req = fmax(req, fabs(r));
        theta += fabs(r);
      }
    } else {
      // (the last stage has no defect, but the recursion reads the entries -- times a zero cost-to-go; records in
      //  LDS start from whatever the previous kernel left there, and 0 * NaN is not 0)
#pragma unroll
      for (int j = 0; j < NX; j++) rec[C::R_RC + j] = 0.0;
    }
    if constexpr (EARLY) {
      for_range<0, NQ>(finalize_var);
      if constexpr (NS > 0) finalize_var(std::integral_constant<int, NX>{});
    } else {
      for_range<0, NV>(finalize_var);
    }
  } else {
#pragma unroll
    for (int j = 0; j < NV; j++) rs[j] += gf[j];
    if (k < N - 1) {
      double xn[NX];
      double A5[25], B5[10];
      diffdrive_step<C>(M.dt, z, xn, A5, B5, true);
      constexpr int map[5] = {0, 1, 2, 6, 7};
#pragma unroll
      for (int i = 0; i < 25; i++) rec[C::R_A5 + i] = A5[i];
#pragma unroll
      for (int i = 0; i < 10; i++) rec[C::R_B5 + i] = B5[i];
      {
        // nu . grad^2 Phi of the discrete dynamics (ERK2 midpoint, 5 nodes; closed form of diffdrive_step):
        // x+ = x + h sum_n cos(al_n) be_n, y+ = y + h sum_n sin(al_n) be_n, al_n = theta + a_n omega + b_n u1,
        // be_n = v + a_n u0, a_n = (n + 1/2) h, b_n = h^2 n (n + 1) / 2 -- only the costates of x and y carry curvature:
        // D = h sum_n [(-nx cos - ny sin) be_n ga ga^T + (-nx sin + ny cos)(ga gb^T + gb ga^T)], ga = (1, a_n, b_n) over
        // (theta, omega, u1), gb = (1, a_n) over (v, u0).  Stored negated (the recursion subtracts cwt x the entry).
        const double hn = M.dt / kErkNodes;
        const double th = z[2], vv = z[6], om = z[7], u0 = z[NX + NS], u1 = z[NX + NS + 1];
        double Dd[C::ND + 1];
#pragma unroll
        for (int i = 0; i <= C::ND; i++) Dd[i] = 0.0;
#pragma unroll 1
        for (int nn_ = 0; nn_ < kErkNodes; nn_++) {
          const double an = (nn_ + 0.5) * hn, bn = hn * hn * (double)(nn_ * (nn_ + 1)) * 0.5;
          double sn, cn;
          sincos(th + an * om + bn * u1, &sn, &cn);
          const double be = vv + an * u0;
          const double Pn = hn * (-nun[0] * cn - nun[1] * sn) * be, Sn = hn * (-nun[0] * sn + nun[1] * cn);
          Dd[0] += Pn * an; Dd[1] += Pn * bn; Dd[2] += Pn * an * an; Dd[3] += Pn * an * bn; Dd[4] += Pn * bn * bn;
          Dd[5] += Sn; Dd[6] += Sn * an; Dd[7] += Sn * an; Dd[8] += Sn * an * an; Dd[9] += Sn * bn; Dd[10] += Sn * bn * an;
          Dd[C::ND] += Pn;   // (theta, theta): into the q block
        }
#pragma unroll
        for (int i = 0; i < C::ND; i++) rec[C::R_D + i] = M.use_curv ? -Dd[i] : 0.0;
        Cqq[2][2] -= M.use_curv ? Dd[C::ND] : 0.0;
      }
      // A = I outside the reduced block
#pragma unroll
      for (int j = 3; j < 6; j++) rs[j] += nun[j];
#pragma unroll
      for (int c = 0; c < 5; c++) {
        double acc = 0;
#pragma unroll
        for (int r = 0; r < 5; r++) acc += A5[r * 5 + c] * nun[map[r]];
        rs[map[c]] += acc;
      }
#pragma unroll
      for (int c = 0; c < 2; c++) {
        double acc = 0;
#pragma unroll
        for (int r = 0; r < 5; r++) acc += B5[r * 2 + c] * nun[map[r]];
        rs[NX + NS + c] += acc;
      }
#pragma unroll
      for (int j = 0; j < NX; j++) {
        const double r = xn[j] - xk1[j];
        rec[C::R_RC + j] = r;
        req = fmax(req, fabs(r));
        theta += fabs(r);
      }
    } else {
      // (see the holonomic chain: every entry the recursion reads is written)
#pragma unroll
      for (int i = 0; i < 35 + C::ND; i++) rec[C::R_A5 + i] = 0.0;
#pragma unroll
      for (int j = 0; j < NX; j++) rec[C::R_RC + j] = 0.0;
    }
#pragma unroll
    for (int j = 0; j < NV; j++) {
      double r = rs[j];
      if (j < NX) {
        if (k == 0) continue;  // x_1 is fixed: no stationarity condition
        r -= nuk[j];
      }
      rstat = fmax(rstat, fabs(r));
    }
#pragma unroll
    for (int j = NQ; j < NV; j++) rec[C::R_DG + j - NQ] = Dg[j];
    if constexpr (NS > 0) {
#pragma unroll
      for (int j = 0; j < NV; j++) rec[C::R_CS + j] = cs[j];
    }
#pragma unroll
    for (int j = 0; j < NV; j++) {
      rec[C::R_Q0 + j] = gf[j] + q0[j];
      rec[C::R_Q1 + j] = q1[j];
      gfa[IDXL(j)] = gf[j];
    }
  }

  // ---- write the q block of the condensed stage ------------------------------------------
  {
    int s = 0;
#pragma unroll
    for (int a = 0; a < NQ; a++)
#pragma unroll
      for (int c = a; c < NQ; c++) {
        if constexpr (QLDS) rec[C::R_Q + s] = qacc[s * kSweepBlock];
        else rec[C::R_Q + s] = Qqq[a][c];
        s++;
      }
  }
  {
    // (zero when the model or this solve does not use the curvature terms: k_riccati reads the slot regardless)
    int s = 0;
#pragma unroll
    for (int a = 0; a < NQ; a++)
#pragma unroll
      for (int c = a; c < NQ; c++) {
        if constexpr (QLDS) rec[C::R_C + s] = M.use_curv ? (double)qacc[(C::NQ2 + s) * kSweepBlock] : 0.0;
        else rec[C::R_C + s] = (QC && M.use_curv) ? Cqq[QC ? a : 0][QC ? c : 0] : 0.0;
        s++;
      }
  }
  rec[C::R_ZERO] = 0.0;
  const double logsum = log(lprod) + 0.6931471805599453094 * (double)lexp;
  bad |= (int)(!isfinite(f) | !isfinite(theta) | !isfinite(logsum));
  st(3);
  st.put(out, 0, 4);
  out.f = f; out.th = theta; out.logs = logsum; out.rstat = rstat; out.req = req; out.rineq = rineq;
  out.rcomp = rcomp; out.sumc = sumc; out.minc = minc; out.bad = (double)bad;
}

template <class C, class V>
__global__ __launch_bounds__(kSweepBlock, C::SWEEP_WPE) void k_sweep(const DevModel M, const DevTables *__restrict__ Tp, const Ws W,
                                               const int B, const int first, const int warm) {
  SecStamps st;   // [0 .. 3] the sections of sweep_body, [4] the whole kernel
  st.start();
  const int gid = blockIdx.x * kSweepBlock + threadIdx.x;
  const int li = gid % W.Bp;   // position in the compacted list of iterating instances
  // (Bp % 64 == 0: the stage is the same for the 64 lanes of a wavefront; as a scalar, every test on it is a scalar
  //  branch taken by the whole wavefront instead of a masked region)
  const int k = __builtin_amdgcn_readfirstlane(gid / W.Bp);
  if (li >= *W.n_act || k >= M.N) return;
  const int b = W.act_idx[li];
  if (W.status[b] != ST_ACTIVE) return;
  const int N = M.N;
  (void)B;
  const int cur = W.cur[b], nxt = cur ^ 1;
  SweepIO<gdouble> io;
  io.zc = (gdouble *)W.z[cur]; io.tc = (gdouble *)W.t[cur]; io.lc = (gdouble *)W.lam[cur]; io.nc = (gdouble *)W.nu[cur];
  io.zn = (gdouble *)W.z[nxt]; io.tn = (gdouble *)W.t[nxt]; io.ln = (gdouble *)W.lam[nxt]; io.nn = (gdouble *)W.nu[nxt];
  io.pp = (gdouble *)W.p; io.dzp = (gdouble *)W.dz; io.gro = (gdouble *)W.grow[cur]; io.jqo = (gdouble *)W.Jq[cur];
  io.grn = (gdouble *)W.grow[nxt]; io.jqn = (gdouble *)W.Jq[nxt];
  io.nup = (gdouble *)W.nunew; io.gfa = (gdouble *)W.gfa;
  io.rec = (gdouble *)(W.R + ((size_t)b * N + k) * C::RS);   // this lane's stage record
  // element offset of this lane inside a slot (32-bit, so that accesses become uniform base + lane offset) and slot size
  io.loff = (unsigned)k * (unsigned)W.Bp + (unsigned)b;
  io.kstride = (unsigned)W.Bp;
  io.SS = (size_t)N * W.Bp;
  io.SSd = io.SS; io.loffd = io.loff; io.kstrided = io.kstride;
  io.wl = (gdouble *)W.wlam; io.wn = (gdouble *)W.wnu;
  io.warm = warm;   // (wave uniform; instances without usable multipliers hold zeros and mu0 in the warm arrays)
  // ---- step lengths of this trial --------------------------------------
  // null pass: the current point is re-evaluated unchanged so that the step can be
  // recomputed with the Gauss-Newton blocks (fallback of a failed curvature step)
  const bool nostep = first || (W.redo[b] != 0);
  double alpha = 0.0, adual = 0.0;
  if (!nostep) {
    alpha = ldexp(__longlong_as_double((long long)W.amin_p[b]), -W.ls[b]);
    adual = __longlong_as_double((long long)W.amin_d[b]);
  }
  Partials pt;
  const V v(M, *Tp);
  const SweepK sk = {M.N, M.dt, M.use_curv};
  __shared__ double sq[C::FKCURV ? (2 * C::NQ2 + C::NX + C::NQ) * kSweepBlock : 1];
  ldouble *const qacc = (ldouble *)sq + threadIdx.x;
  if (first) sweep_body<C, -1, gdouble, V, 1>(sk, v, io, k, true, nostep, alpha, adual, W.mu[b], pt, qacc);
  else sweep_body<C, -1, gdouble, V, 0>(sk, v, io, k, false, nostep, alpha, adual, W.mu[b], pt, qacc);
  const unsigned loff = io.loff;
  const size_t SS = io.SS;
  W.part[IDXL(P_F)] = pt.f;
  W.part[IDXL(P_TH)] = pt.th;
  W.part[IDXL(P_LOGS)] = pt.logs;
  W.part[IDXL(P_RSTAT)] = pt.rstat;
  W.part[IDXL(P_REQ)] = pt.req;
  W.part[IDXL(P_RINEQ)] = pt.rineq;
  W.part[IDXL(P_RCOMP)] = pt.rcomp;
  W.part[IDXL(P_SUMC)] = pt.sumc;
  W.part[IDXL(P_MINC)] = pt.minc;
  W.part[IDXL(P_BAD)] = pt.bad;
  st(4);
  st.get(pt, 0, 4);
  st.flush((threadIdx.x & 63) == 0, 5);
}

// ===========================================================================
// k_riccati: per-instance decisions + block-tridiagonal Riccati recursion
// ===========================================================================
// One 64-lane wavefront per instance.  The stage matrices live in LDS and every
// small dense operation of the recursion is spread over the lanes (one output
// entry per lane and pass), so the dependent chain per stage is a handful of
// LDS round trips instead of ~1500 serial fp64 instructions of one lane.
//   backward, stage k:  fill Q_k, q_k      (compact blocks -> dense (nx+nw)^2, lanes over entries)
//                       T = P [A|B], Pc = P rc + p
//                       Q += [A|B]^T T, q += [A|B]^T Pc
//                       Cholesky of Qww (every lane, registers), gains K | kff (one column per lane)
//                       P = sym(Qxx + Qxw K), p = qx + Qxw kff
//   forward, stage k:   dw = K dx + kff, nu+ = P dx + p, dx+ = [A|B][dx; dw] + rc
template <int NW>
__device__ __forceinline__ void chol_solve(const double (&L)[NW][NW], const double (&invd)[NW], double (&v)[NW]) {
  // L L^T x = v with the reciprocals of the diagonal supplied (no divisions on the chain)
#pragma unroll
  for (int i = 0; i < NW; i++) {
    double s = v[i];
#pragma unroll
    for (int l = 0; l < i; l++) s -= L[i][l] * v[l];
    v[i] = s * invd[i];
  }
#pragma unroll
  for (int i = NW - 1; i >= 0; i--) {
    double s = v[i];
#pragma unroll
    for (int l = i + 1; l < NW; l++) s -= L[l][i] * v[l];
    v[i] = s * invd[i];
  }
}

// LDS hand-off inside ONE wavefront: DS instructions of a wave execute in issue order, so a
// compiler-level ordering point is all that is needed (a __syncthreads() would also drain the
// global loads that are deliberately left in flight as the next stage's prefetch).
#define WSYNC()                                              \
  do {                                                       \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
    __builtin_amdgcn_wave_barrier();                         \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
  } while (0)

// reductions over the LPI consecutive lanes that work on one instance (a whole wavefront or half of one)
template <int LPI>
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = LPI / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
template <int LPI>
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = LPI / 2; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}
template <int LPI>
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = LPI / 2; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
  return v;
}

// Several reductions at once, step by step: the exchanges of one step of all of them are issued together (a single
// reduction is a chain of dependent LDS-crossbar round trips; done one after the other, eleven of them cost eleven
// chains).  Same partner pattern, hence the same rounding, as wave_sum / wave_max / wave_min.
template <int LPI, int NS_, int NM_, int NN_>
__device__ __forceinline__ void wave_reduce_many(double (&sums)[NS_], double (&maxs)[NM_], double (&mins)[NN_]) {
#pragma unroll
  for (int off = LPI / 2; off >= 1; off >>= 1) {
    double ts[NS_], tm[NM_], tn[NN_];
#pragma unroll
    for (int i = 0; i < NS_; i++) ts[i] = __shfl_xor(sums[i], off, 64);
#pragma unroll
    for (int i = 0; i < NM_; i++) tm[i] = __shfl_xor(maxs[i], off, 64);
#pragma unroll
    for (int i = 0; i < NN_; i++) tn[i] = __shfl_xor(mins[i], off, 64);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NS_; i++) sums[i] += ts[i];
#pragma unroll
    for (int i = 0; i < NM_; i++) maxs[i] = fmax(maxs[i], tm[i]);
#pragma unroll
    for (int i = 0; i < NN_; i++) mins[i] = fmin(mins[i], tn[i]);
  }
}

// ---- per-instance solver state ------------------------------------------------------------------------
// One set of words per instance.  The pass kernels keep them in the workspace (arrays over the batch), the
// fused kernel in registers of the wavefront that owns the instance; the decision logic is the same code.
struct Inst {
  double mu, rho, phi0, Dd, fcur, thcur, logcur, res_stat, res_eq, res_ineq, res_comp, obj;
  double amin_p, amin_d;   // fraction-to-the-boundary step lengths of the current step
  double mu_hold;          // barrier restart: the level mu is held at (0: none)
  int status, iters, ls, ls0, lsst, cur, newstep, redo, force_gn, gn_sticky, curv_fail, usedc, stall, curv_skip, curv_back;
  int small_steps;         // barrier restart: accepted short steps in a row
  double theta_mem, theta_c;      // scaled curvature: the scale the next curvature step starts from / of this iteration
  int theta_clean, theta_retry;   // accepted curvature steps in a row without a retry / this iteration has retried
};
__device__ __forceinline__ void inst_init(Inst &s, double mu0) {
  s.mu = mu0; s.rho = 0.0; s.phi0 = 0.0; s.Dd = 0.0; s.fcur = 0.0; s.thcur = 0.0; s.logcur = 0.0;
  s.res_stat = 0.0; s.res_eq = 0.0; s.res_ineq = 0.0; s.res_comp = 0.0; s.obj = 0.0;
  s.amin_p = 1.0; s.amin_d = 1.0;
  s.status = ST_ACTIVE; s.iters = 0; s.ls = 0; s.ls0 = 0; s.lsst = 0; s.cur = 0; s.newstep = 0; s.redo = 0;
  s.force_gn = 0; s.gn_sticky = 0; s.curv_fail = 0; s.usedc = 0; s.stall = 0; s.curv_skip = 0; s.curv_back = 0;
  s.small_steps = 0; s.mu_hold = 0.0;
  s.theta_mem = 1.0; s.theta_c = 1.0; s.theta_clean = 0; s.theta_retry = 0;
}
__device__ __forceinline__ void inst_load(Inst &s, const Ws &W, int b) {
  s.mu = W.mu[b]; s.rho = W.rho[b]; s.phi0 = W.phi0[b]; s.Dd = W.Dd[b]; s.fcur = W.fcur[b]; s.thcur = W.thcur[b];
  s.logcur = W.logcur[b]; s.res_stat = W.res_stat[b]; s.res_eq = W.res_eq[b]; s.res_ineq = W.res_ineq[b];
  s.res_comp = W.res_comp[b]; s.obj = W.obj[b];
  s.amin_p = __longlong_as_double((long long)W.amin_p[b]); s.amin_d = __longlong_as_double((long long)W.amin_d[b]);
  s.status = W.status[b]; s.iters = W.iters[b]; s.ls = W.ls[b]; s.ls0 = W.ls0[b]; s.lsst = W.lsst[b]; s.cur = W.cur[b];
  s.newstep = W.newstep[b]; s.redo = W.redo[b]; s.force_gn = W.force_gn[b]; s.gn_sticky = W.gn_sticky[b];
  s.curv_fail = W.curv_fail[b]; s.usedc = W.usedc[b]; s.stall = W.stall[b]; s.curv_skip = W.curv_skip[b]; s.curv_back = W.curv_back[b];
  s.small_steps = W.small_steps[b]; s.mu_hold = W.mu_hold[b];
  s.theta_mem = W.theta_mem[b]; s.theta_c = W.theta_c[b]; s.theta_clean = W.theta_clean[b]; s.theta_retry = W.theta_retry[b];
}
__device__ __forceinline__ void inst_store(const Inst &s, const Ws &W, int b) {
  W.mu[b] = s.mu; W.rho[b] = s.rho; W.phi0[b] = s.phi0; W.Dd[b] = s.Dd; W.fcur[b] = s.fcur; W.thcur[b] = s.thcur;
  W.logcur[b] = s.logcur; W.res_stat[b] = s.res_stat; W.res_eq[b] = s.res_eq; W.res_ineq[b] = s.res_ineq;
  W.res_comp[b] = s.res_comp; W.obj[b] = s.obj;
  W.amin_p[b] = (unsigned long long)__double_as_longlong(s.amin_p); W.amin_d[b] = (unsigned long long)__double_as_longlong(s.amin_d);
  W.status[b] = s.status; W.iters[b] = s.iters; W.ls[b] = s.ls; W.ls0[b] = s.ls0; W.lsst[b] = s.lsst; W.cur[b] = s.cur;
  W.newstep[b] = s.newstep; W.redo[b] = s.redo; W.force_gn[b] = s.force_gn; W.gn_sticky[b] = s.gn_sticky;
  W.curv_fail[b] = s.curv_fail; W.usedc[b] = s.usedc; W.stall[b] = s.stall; W.curv_skip[b] = s.curv_skip; W.curv_back[b] = s.curv_back;
  W.small_steps[b] = s.small_steps; W.mu_hold[b] = s.mu_hold;
  W.theta_mem[b] = s.theta_mem; W.theta_c[b] = s.theta_c; W.theta_clean[b] = s.theta_clean; W.theta_retry[b] = s.theta_retry;
}

// whole-horizon sums / maxima of the trial point the last sweep evaluated (+ the merit slope of the step)
struct Reduced { double f, th, lgs, rstat, req, rineq, rcomp, sumc, minc, badf, gphi; };

// Armijo test of the trial point, acceptance, barrier update, convergence tests.  Returns true when a new
// step has to be computed (Riccati recursion next; `usec`: with the exact constraint curvature); false when
// the instance retries with a shorter step, re-evaluates (null pass) or has stopped (s.status).
template <class C>
__device__ __forceinline__ bool inst_decide(const DevModel &M, Inst &s, const Reduced &r, const bool first, bool &usec) {
  const int N = M.N;
  s.newstep = 0;
  double mu = s.mu;
  int status = ST_ACTIVE;
  int iters = s.iters;
  const bool redo = (!first) && (s.redo != 0);
  int lsst = first ? 0 : s.lsst;
  double alpha_acc = 1.0;   // length of the step accepted in this pass (barrier restart)
  usec = false;
  if (first) {
    if (r.badf != 0.0) status = -7;  // inverse-barrier row not strictly feasible at the start
  } else if (redo) {
    // null pass: same point, the step is recomputed below with the Gauss-Newton blocks
    s.redo = 0;
  } else {
    const double a0 = s.amin_p;
    int ls = s.ls;
    double rho = s.rho, phi0 = s.phi0, Dd = s.Dd;
    if (ls == s.ls0) {   // first trial of this line search
      const double thc = s.thcur;
      if (thc > 1e-13) {
        const double need = r.gphi / (0.9 * thc);
        if (rho < need) rho = need + 1.0;
      }
      Dd = r.gphi - rho * thc;
      phi0 = s.fcur - mu * s.logcur + rho * thc;
      s.rho = rho; s.phi0 = phi0; s.Dd = Dd;
    }
    const double alpha = ldexp(a0, -ls);
    const double phi = r.f - mu * r.lgs + rho * r.th;
    const bool ok = (r.badf == 0.0) && (phi <= phi0 + kArmijo * alpha * Dd + 1e-13 * fabs(phi0));
    const int usedc = s.usedc;
    if (!ok) {
      ls++;
      if (ls > (usedc ? kLsCurv - 1 : M.ls_max)) {
        if (usedc) {
          // the curvature step failed its line search: recompute this iteration's step with
          // the Gauss-Newton blocks (null pass next); latch after repeated failures
          if constexpr (C::BACKOFF) {
            // (the unicycle, the small chains: the next curvature steps are skipped -- 1, 2, 4 .. 16 iterations, doubling
            //  with every failure in a row, over after a success -- instead of a latch: DESIGN.md 3)
            s.curv_back = s.curv_back ? (s.curv_back < kCurvBackMax ? 2 * s.curv_back : kCurvBackMax) : 1;
            s.curv_skip = s.curv_back;
          } else {
            const int cf = s.curv_fail + 1;
            s.curv_fail = cf;
            if (cf >= kCurvFailMax) s.gn_sticky = 1;
          }
          s.redo = 1;
          s.force_gn = 1;
          s.ls = 0;
          return false;
        }
        s.status = -8;  // line search failure; the current iterate is returned
        return false;
      }
      s.ls = ls;
      return false;  // next sweep retries with alpha / 2
    }
    if (usedc) { s.curv_fail = 0; s.curv_back = 0; }
    if constexpr (C::CSCALE) {
      // scaled curvature: the scale that needed a retry is kept, kCsClean accepted curvature steps in a row without a
      // retry double it again; an iteration whose retries all failed (Gauss-Newton step accepted) keeps the last scale
      if (usedc) {
        if (s.theta_retry) { s.theta_mem = s.theta_c; s.theta_clean = 0; }
        else if (++s.theta_clean >= kCsClean) { s.theta_mem = s.theta_c < 0.75 ? 2.0 * s.theta_c : 1.0; s.theta_clean = 0; }
      } else if (s.theta_retry) { s.theta_mem = s.theta_c; s.theta_clean = 0; }
    }
    // the arms: a Gauss-Newton step accepted at full length releases the latch (the failures that set it belong to
    // the first iterations of a warm start, where the fraction to the boundary cuts the steps)
    if constexpr (C::FKCURV) {
      if (!usedc && ls == 0) { s.gn_sticky = 0; s.curv_fail = 0; }
    }
    // step-length memory: the next Gauss-Newton line search starts one halving above the accepted one (models
    // whose steps overshoot every iteration -- the unicycle -- otherwise pay a pass per halving per iteration)
    lsst = ls > kLsGrow ? ls - kLsGrow : 0;
    s.lsst = lsst;
    alpha_acc = alpha;
    iters++;
  }
  // ---- accept the trial point ------------------------------------------------------
  if (status == ST_ACTIVE) {
    const double f_prev = s.fcur;
    const int stall0 = s.stall;
    s.cur ^= 1;
    s.fcur = r.f;
    s.thcur = r.th;
    s.logcur = r.lgs;
    if (!redo) {
      s.iters = iters;
      s.res_stat = r.rstat; s.res_eq = r.req; s.res_ineq = r.rineq; s.res_comp = r.rcomp; s.obj = r.f;
      if (!first) {
        // LOQO-style centrality rule with floors (DESIGN.md, section "Algorithm")
        const double cnt = (double)N * (double)M.m;
        const double avg = r.sumc / cnt;
        const double xi = r.minc / avg;
        double sg = 0.05 * (1.0 - xi) / xi;
        if (sg > 2.0) sg = 2.0;
        sg = 0.1 * sg * sg * sg;
        if (sg < 0.02) sg = 0.02;
        if (sg > 0.8) sg = 0.8;
        mu = sg * avg;
        if (mu < 0.1 * M.tol_comp) mu = 0.1 * M.tol_comp;
        // barrier restart on stalled steps (oracle: ORC_RS_*): from iteration kRsIt on, kRsN accepted steps in
        // a row shorter than kRsAlpha while mu < kRsMu -- the iterate crawls along a boundary with the barrier at its
        // floor -- hold mu at kRsMu, released by the factor kRsDecay per iteration
        {
          int ss = (iters - 1 >= kRsIt && alpha_acc < kRsAlpha) ? s.small_steps + 1 : 0;
          double mh = s.mu_hold;
          if (ss >= kRsN && mu < kRsMu && !(mh > 0.0)) { mh = kRsMu; ss = 0; }
          if (mh > 0.0) {
            if (mu < mh) mu = mh;
            mh *= kRsDecay;
            if (mh < 0.1 * M.tol_comp) mh = 0.0;
          }
          s.small_steps = ss; s.mu_hold = mh;
        }
        s.mu = mu;
        if (!(mu < kMuDiverged)) status = -7;
      }
      if (status == ST_ACTIVE) {
        if (!isfinite(r.rstat) || !isfinite(r.req) || !isfinite(r.rineq)) status = -6;
        else if (r.rstat <= M.tol_stat && r.req <= M.tol_eq && r.rineq <= M.tol_ineq && r.rcomp <= kCompFrac * M.tol_comp) status = 1;
        else {
          // acceptable termination: feasible, complementary, objective stagnant for acc_iters iterations
          int stall = stall0;
          if (!first && r.req <= kAccFeas && r.rineq <= kAccFeas && r.rcomp <= kAccFeas &&
              fabs(r.f - f_prev) <= M.acc_obj_tol * fmax(1.0, fabs(r.f)))
            stall++;
          else
            stall = 0;
          s.stall = stall;
          if (M.acc_iters > 0 && stall >= M.acc_iters) status = 2;
          else if (iters >= M.max_iter) status = 0;
        }
      }
    }
  }
  if (status != ST_ACTIVE) {
    s.status = status;
    return false;
  }
  // exact constraint curvature unless latched off or this is the fallback pass
  if constexpr (C::CURV || C::DDCURV) usec = M.use_curv && !s.gn_sticky && !s.force_gn && (mu <= kCurvMu);
  if constexpr (C::BACKOFF) {
    // (a fallback pass -- force_gn -- is not an iteration of its own: the skip counter moves once per iteration)
    if (usec && s.curv_skip > 0) { s.curv_skip--; usec = false; }
  }
  s.force_gn = 0;
  if constexpr (C::CSCALE) {
    if (!redo) { s.theta_c = s.theta_mem; s.theta_retry = 0; }   // (a null pass belongs to the iteration that asked for it)
  }
  // a step with the exact curvature is tried at full length first
  const int lsb = usec ? 0 : lsst;
  s.ls = lsb;
  s.ls0 = lsb;
  return true;
}
// after the recursion: a failed factorisation either falls back to Gauss-Newton (null pass) or stops the instance
__device__ __forceinline__ void inst_after_recursion(Inst &s, const bool chol_ok, const bool usec, const bool backoff = false,
                                                     const bool cscale = false) {
  if (!chol_ok) {
    if (usec) {
      if (cscale && s.theta_c > kCsMin) {
        // scaled curvature: the same iteration again (null pass next) with the curvature terms at half their weight
        s.theta_c *= 0.5; s.theta_retry = 1; s.redo = 1; s.usedc = 0;
        return;
      }
      if (backoff) {   // (diff-drive: see inst_decide)
        s.curv_back = s.curv_back ? (s.curv_back < kCurvBackMax ? 2 * s.curv_back : kCurvBackMax) : 1;
        s.curv_skip = s.curv_back;
      }
      // reduced Hessian not positive definite with the curvature terms: recompute this
      // iteration's step with the Gauss-Newton blocks (null pass next); not counted as a
      // line-search failure
      s.redo = 1; s.force_gn = 1; s.usedc = 0;
      return;
    }
    s.status = -5;
    return;
  }
  s.usedc = usec ? 1 : 0;
  s.newstep = 1;
  s.amin_p = 1.0;   // the step kernel takes the minima next
  s.amin_d = 1.0;
}

// where the recursion leaves the step: dz[slot * SS + k * KS], nunew likewise (pointers advanced to the instance)
template <class RP = gdouble>
struct StepOut {
  RP *dz, *nunew;
  size_t SS, KS;
};

// v moved between lanes by a DPP control word (quad permutations, row mirrors): full-rate vector moves, no LDS
// crossbar round trip.  Every lane of the 8 aligned lanes a reader belongs to must be active: the control words in use
// (quad permutations, row_half_mirror) read only those, so the `old` operand of the move is never taken -- it is left
// undefined, with bound_ctrl, and no instruction is spent on setting it (a zero cost two v_mov_b32 per move).
template <int CTRL>
__device__ __forceinline__ double dpp_move(const double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// Address of a per-lane LDS access that moves with the stage: base + k * strb bytes (k uniform, below 2^24).  A lane
// without that access has stride 0 and a word of its own as base: one v_mad_u32_u24, no select.
typedef __attribute__((address_space(3))) char lbyte;
__device__ __forceinline__ ldouble *stage_ptr(ldouble *const base, const unsigned strb, const int k) {
  return (ldouble *)((lbyte *)base + __umul24((unsigned)k, strb));
}

#include "rmpc_riccati.hpp"   // the Riccati recursion (riccati_recursion: one function per path)

template <class C, int IPB>
__global__ __launch_bounds__(64 * IPB, C::RIC_WPE) void k_riccati(const DevModel M, const Ws W, const int B, const int first,
                                                const int pass) {
  // IPB wavefronts per block work on IPB consecutive list entries: neighbouring instances share
  // the 128-byte lines of the batch-minor arrays, so most of a wave's requests hit the CU's L1
  // Two instantiations are launched every pass and pick their regime from the list length:
  // the grouped one (IPB = C::IPB) while many instances iterate, the one-wave blocks (IPB = 1,
  // static LDS addresses, lowest latency) in the iteration tail.
  const int nact = *W.n_act;
  if constexpr (C::IPB > 1) {
    if ((IPB > 1) != (nact >= kGroupedMin)) return;
  }
  // lanes per instance: a whole wavefront, or half of one in the grouped regime of the small models (their
  // dense blocks have few rows: two instances per wavefront halve the LDS instructions an instance costs, and
  // LDS instruction throughput is what bounds this kernel when the whole batch iterates)
  constexpr int LPI = (IPB > 1) ? C::RIC_LPI : 64;
  constexpr int IPW = 64 / LPI;
  const int wv = threadIdx.x / LPI;   // instance slot within the block
  const int li = blockIdx.x * (IPB * IPW) + wv;
  if (li >= nact) return;
  const int b = W.act_idx[li];
  if (W.status[b] != ST_ACTIVE) return;  // uniform over the lanes of an instance (whole wavefront, or one half in the grouped regime)
  const int lane = threadIdx.x & (LPI - 1);
  const int N = M.N;
  (void)B; (void)pass;

  // ---- reduce the stage partials of the trial point --------------------------------
  Reduced r = {0, 0, 0, 0, 0, 0, 0, 0, 1e300, 0, 0};
  for (int k = lane; k < N; k += LPI) {
    r.f += W.part[IDX(P_F, k, b)];
    r.th += W.part[IDX(P_TH, k, b)];
    r.lgs += W.part[IDX(P_LOGS, k, b)];
    r.rstat = fmax(r.rstat, W.part[IDX(P_RSTAT, k, b)]);
    r.req = fmax(r.req, W.part[IDX(P_REQ, k, b)]);
    r.rineq = fmax(r.rineq, W.part[IDX(P_RINEQ, k, b)]);
    r.rcomp = fmax(r.rcomp, W.part[IDX(P_RCOMP, k, b)]);
    r.sumc += W.part[IDX(P_SUMC, k, b)];
    r.minc = fmin(r.minc, W.part[IDX(P_MINC, k, b)]);
    r.badf += W.part[IDX(P_BAD, k, b)];
    r.gphi += first ? 0.0 : W.gphi[(size_t)k * W.Bp + b];
  }
  {
    // (all quantities through the xor tree together, step by step: 6 exchange rounds instead of 11 x 6 dependent ones;
    //  the same trees as wave_sum / wave_max / wave_min)
    double rs6[6] = {r.f, r.th, r.lgs, r.sumc, r.badf, r.gphi}, rm4[4] = {r.rstat, r.req, r.rineq, r.rcomp}, rn1[1] = {r.minc};
    wave_reduce_many<LPI>(rs6, rm4, rn1);
    r.f = rs6[0]; r.th = rs6[1]; r.lgs = rs6[2]; r.sumc = rs6[3]; r.badf = rs6[4]; r.gphi = rs6[5];
    r.rstat = rm4[0]; r.req = rm4[1]; r.rineq = rm4[2]; r.rcomp = rm4[3]; r.minc = rn1[0];
  }

  // ---- decisions: every lane computes them (identical values), lane 0 stores ---------
  const bool L0 = (lane == 0);
  Inst s;
  inst_load(s, W, b);
  bool usec = false;
  const bool recurse = inst_decide<C>(M, s, r, first != 0, usec);
  if (L0) inst_store(s, W, b);   // (every lane has loaded the words above: same wavefront, program order)
  if (!recurse) return;
  const double mu = s.mu;        // nothing else of the instance state stays live across the recursion
  __shared__ double lds[IPB * IPW][RicLds<C, LPI>::LDSW];
  constexpr int IMGW = RicLds<C, LPI>::IMG_SLOTS * RicLds<C, LPI>::KPW;
  __shared__ double limg[IMGW > 0 ? IMGW : 1];   // (the arms: gain images of the first IMG_SLOTS stages, one-wavefront blocks)
  static_assert(IMGW == 0 || IPB * IPW == 1, "image slots: one instance per block");
  StepOut<gdouble> so;
  so.dz = (gdouble *)(W.dz + b); so.nunew = (gdouble *)(W.nunew + b); so.SS = (size_t)N * W.Bp; so.KS = (size_t)W.Bp;
  const double cw = usec ? (C::CSCALE ? s.theta_c : 1.0) : 0.0;
  const bool chol_ok = riccati_recursion<C, LPI, false, gdouble>(M.N, M.dt, mu, cw, lane, (ldouble *)lds[wv],
                                                                 (const gdouble *)(W.R + (size_t)b * N * C::RS),
                                                                 (gdouble *)(W.KP + (size_t)b * N * W.kps), W.kps, so,
                                                                 nullptr, (ldouble *)limg);
  if (L0) {
    // = inst_after_recursion on the stored words
    if (!chol_ok) {
      if (usec) {
        if (C::CSCALE && s.theta_c > kCsMin) {   // scaled curvature: the iteration again at half the weight
          W.theta_c[b] = 0.5 * s.theta_c; W.theta_retry[b] = 1; W.redo[b] = 1; W.usedc[b] = 0;
        } else {
          W.redo[b] = 1; W.force_gn[b] = 1; W.usedc[b] = 0;
          if constexpr (C::BACKOFF) {
            const int cb = s.curv_back ? (s.curv_back < kCurvBackMax ? 2 * s.curv_back : kCurvBackMax) : 1;
            W.curv_back[b] = cb; W.curv_skip[b] = cb;
          }
        }
      }
      else W.status[b] = -5;
    } else {
      W.usedc[b] = usec ? 1 : 0;
      W.newstep[b] = 1;
      W.amin_p[b] = (unsigned long long)__double_as_longlong(1.0);  // k_step takes the minima next
      W.amin_d[b] = (unsigned long long)__double_as_longlong(1.0);
    }
  }
}

// ===========================================================================
// k_riccati_lane: the same decisions and recursion with ONE LANE PER INSTANCE
// ===========================================================================
// The "tiny batched" layout of the recursion (round 3, review item 1a): 64 instances per wavefront, the cost-to-go,
// the dense stage block and the gains of an instance in its lane's registers, no LDS, no exchange between lanes; a
// stage is a few hundred dependent-free multiply-adds per lane.  A wavefront costs the same ~900 instructions per
// stage whether 2 or 64 of its lanes hold an instance, so the layout pays once the batch fills wavefronts that would
// otherwise each carry one instance: it is selected for lists of at least kLaneMin instances (holonomic chains with
// n <= 3; the arm's blocks do not fit a lane's registers), k_riccati's one-instance-per-wavefront blocks below that.
// Same arithmetic per entry as riccati_recursion's generic path (closed-form [A|B]^T P [A|B], Cholesky with Newton
// reciprocal square roots, symmetrised cost-to-go); the stage partials are summed in stage order instead of by a
// shuffle tree (a rounding-level difference in the merit value).
constexpr int kLaneMin = 16384;
template <class C>
__global__ __launch_bounds__(64) void k_riccati_lane(const DevModel M, const Ws W, const int B, const int first) {
  constexpr int NQ = C::NQ, NX = C::NX, NS = C::NS, NV = C::NV, NW = C::NW;
  static_assert(C::ROBOT == RMPC_ROBOT_CHAIN && NQ <= 3, "lane-per-instance recursion: small holonomic chains only");
  const int li = blockIdx.x * 64 + threadIdx.x;
  if (li >= *W.n_act) return;
  const int b = W.act_idx[li];
  if (W.status[b] != ST_ACTIVE) return;
  const int N = M.N;
  (void)B;
  Reduced r = {0, 0, 0, 0, 0, 0, 0, 0, 1e300, 0, 0};
  for (int k = 0; k < N; k++) {
    r.f += W.part[IDX(P_F, k, b)];
    r.th += W.part[IDX(P_TH, k, b)];
    r.lgs += W.part[IDX(P_LOGS, k, b)];
    r.rstat = fmax(r.rstat, W.part[IDX(P_RSTAT, k, b)]);
    r.req = fmax(r.req, W.part[IDX(P_REQ, k, b)]);
    r.rineq = fmax(r.rineq, W.part[IDX(P_RINEQ, k, b)]);
    r.rcomp = fmax(r.rcomp, W.part[IDX(P_RCOMP, k, b)]);
    r.sumc += W.part[IDX(P_SUMC, k, b)];
    r.minc = fmin(r.minc, W.part[IDX(P_MINC, k, b)]);
    r.badf += W.part[IDX(P_BAD, k, b)];
    r.gphi += first ? 0.0 : W.gphi[(size_t)k * W.Bp + b];
  }
  Inst s;
  inst_load(s, W, b);
  bool usec = false;
  const bool recurse = inst_decide<C>(M, s, r, first != 0, usec);
  inst_store(s, W, b);
  if (!recurse) return;
  const double mu = s.mu, cwt = usec ? (C::CSCALE ? s.theta_c : 1.0) : 0.0;
  const double h = M.dt, h2 = 0.5 * M.dt * M.dt;
  constexpr int NP2 = NX * (NX + 1) / 2;
  constexpr int OFF_KFF = NW * NX, OFF_PT = NW * NX + NW, OFF_P = OFF_PT + NP2, OFF_RC = OFF_P + NX;
  auto tri = [](int i, int j) __attribute__((always_inline)) {
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    return lo * NX - lo * (lo - 1) / 2 + (hi - lo);
  };
  // kind of a variable (0 q, 1 v, 2 u, 3 slack) and its joint: rows of [A | B]^T are (1, 0), (h, 1), (h2, h) on the
  // (q+, v+) block rows
  auto kind = [](int i) __attribute__((always_inline)) { return i < NQ ? 0 : (i < NX ? 1 : (i >= NX + NS ? 2 : 3)); };
  auto joint = [](int i) __attribute__((always_inline)) { return i < NQ ? i : (i < NX ? i - NQ : (i >= NX + NS ? i - NX - NS : 0)); };
  double P[NX][NX], pv[NX];
#pragma unroll
  for (int i = 0; i < NX; i++) {
    pv[i] = 0.0;
#pragma unroll
    for (int j = 0; j < NX; j++) P[i][j] = 0.0;
  }
  bool chol_ok = true;
  const gdouble *const rb = (const gdouble *)(W.R + (size_t)b * N * C::RS);
  gdouble *const kpb = (gdouble *)(W.KP + (size_t)b * N * W.kps);
  for (int k = N - 1; k >= 0; k--) {
    const gdouble *const rec = rb + (size_t)k * C::RS;
    gdouble *const kpk = kpb + (size_t)k * W.kps;
    const bool rec_cost = k < N - 1;
    double rcv[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) rcv[j] = rec[C::R_RC + j];
    // ---- dense stage block Q (NV x NV) and gradient q ------------------------------------------------------
    double Q[NV][NV], q[NV];
#pragma unroll
    for (int i = 0; i < NV; i++)
#pragma unroll
      for (int j = 0; j < NV; j++) {
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        double v = 0.0;
        if (hi < NQ) {
          const int t = lo * NQ - lo * (lo - 1) / 2 + (hi - lo);
          v = rec[C::R_Q + t] - cwt * (C::CURV ? (double)rec[C::R_C + t] : 0.0);
        } else if (lo == hi) {
          v = rec[C::R_DG + (lo - NQ)];
        } else if (NS > 0 && lo == NX) {
          v = rec[C::R_CS + hi];
        } else if (NS > 0 && hi == NX) {
          v = rec[C::R_CS + lo];
        }
        const int ki = kind(i), kj = kind(j);
        if (ki != 3 && kj != 3) {
          const int ii = joint(i), jj = joint(j);
          const double l1 = ki == 0 ? 1.0 : (ki == 1 ? h : h2), l2 = ki == 0 ? 0.0 : (ki == 1 ? 1.0 : h);
          const double c1 = kj == 0 ? 1.0 : (kj == 1 ? h : h2), c2 = kj == 0 ? 0.0 : (kj == 1 ? 1.0 : h);
          const double add = l1 * (c1 * P[ii][jj] + c2 * P[ii][NQ + jj]) + l2 * (c1 * P[NQ + ii][jj] + c2 * P[NQ + ii][NQ + jj]);
          v += rec_cost ? add : 0.0;
        }
        Q[i][j] = v;
      }
    double Pc[NX];
#pragma unroll
    for (int i = 0; i < NX; i++) {
      double sacc = pv[i];
#pragma unroll
      for (int l = 0; l < NX; l++) sacc += P[i][l] * rcv[l];
      Pc[i] = sacc;
    }
#pragma unroll
    for (int i = 0; i < NV; i++) {
      double v = rec[C::R_Q0 + i] - mu * rec[C::R_Q1 + i];
      const int ki = kind(i);
      if (ki != 3) {
        const int ii = joint(i);
        const double l1 = ki == 0 ? 1.0 : (ki == 1 ? h : h2), l2 = ki == 0 ? 0.0 : (ki == 1 ? 1.0 : h);
        const double add = l1 * Pc[ii] + l2 * Pc[NQ + ii];
        v += rec_cost ? add : 0.0;
      }
      q[i] = v;
    }
    // ---- Cholesky of Qww, gains ----------------------------------------------------------------------------------
    double L[NW][NW], invd[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) {
      double dg = Q[NX + j][NX + j];
#pragma unroll
      for (int l = 0; l < j; l++) dg -= L[j][l] * L[j][l];
      if (!(dg > 0.0)) chol_ok = false;
      double inv = __builtin_amdgcn_rsq(dg);
      inv = inv * (1.5 - 0.5 * dg * inv * inv);
      inv = inv * (1.5 - 0.5 * dg * inv * inv);
      L[j][j] = dg * inv;
      invd[j] = inv;
#pragma unroll
      for (int i = j + 1; i < NW; i++) {
        double sacc = Q[NX + i][NX + j];
#pragma unroll
        for (int l = 0; l < j; l++) sacc -= L[i][l] * L[j][l];
        L[i][j] = sacc * inv;
      }
    }
    double K[NW][NX], kff[NW];
#pragma unroll
    for (int c = 0; c < NX; c++) {
      double col[NW];
#pragma unroll
      for (int i = 0; i < NW; i++) col[i] = -Q[NX + i][c];
      chol_solve<NW>(L, invd, col);
#pragma unroll
      for (int i = 0; i < NW; i++) K[i][c] = col[i];
    }
    {
      double col[NW];
#pragma unroll
      for (int i = 0; i < NW; i++) col[i] = -q[NX + i];
      chol_solve<NW>(L, invd, col);
#pragma unroll
      for (int i = 0; i < NW; i++) kff[i] = col[i];
    }
    // ---- cost-to-go P = sym(Qxx + Qxw K), p = qx + Qxw kff ----------------------------------------------------------
    double Pa[NX][NX];
#pragma unroll
    for (int i = 0; i < NX; i++) {
#pragma unroll
      for (int j = 0; j < NX; j++) {
        double a = Q[i][j];
#pragma unroll
        for (int l = 0; l < NW; l++) a += Q[i][NX + l] * K[l][j];
        Pa[i][j] = a;
      }
      double a = q[i];
#pragma unroll
      for (int l = 0; l < NW; l++) a += Q[i][NX + l] * kff[l];
      pv[i] = a;
    }
#pragma unroll
    for (int i = 0; i < NX; i++)
#pragma unroll
      for (int j = 0; j < NX; j++) P[i][j] = 0.5 * (Pa[i][j] + Pa[j][i]);
    // ---- gain image of the stage: K | kff | P (upper triangle) | p | rc ---------------------------------------------
#pragma unroll
    for (int i = 0; i < NW; i++) {
#pragma unroll
      for (int c = 0; c < NX; c++) kpk[i * NX + c] = K[i][c];
      kpk[OFF_KFF + i] = kff[i];
    }
#pragma unroll
    for (int i = 0; i < NX; i++) {
#pragma unroll
      for (int j = i; j < NX; j++) kpk[OFF_PT + tri(i, j)] = P[i][j];
      kpk[OFF_P + i] = pv[i];
      kpk[OFF_RC + i] = rcv[i];
    }
  }
  if (chol_ok) {
    // ---- forward rollout: dw = kff + K dx, nu+ = p + P dx, dx+ = rc + [A | B][dx; dw] (closed form) --------------
    double dx[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) dx[j] = 0.0;
    const size_t SS = (size_t)N * W.Bp;
    for (int k = 0; k < N; k++) {
      const gdouble *const im = kpb + (size_t)k * W.kps;
      double dw[NW];
#pragma unroll
      for (int i = 0; i < NW; i++) {
        double sacc = im[OFF_KFF + i];
#pragma unroll
        for (int j = 0; j < NX; j++) sacc += im[i * NX + j] * dx[j];
        dw[i] = sacc;
      }
      const size_t o = (size_t)k * W.Bp + b;
#pragma unroll
      for (int j = 0; j < NX; j++) W.dz[(size_t)j * SS + o] = dx[j];
#pragma unroll
      for (int i = 0; i < NW; i++) W.dz[(size_t)(NX + i) * SS + o] = dw[i];
      if (k >= 1) {
#pragma unroll
        for (int i = 0; i < NX; i++) {
          double sacc = im[OFF_P + i];
#pragma unroll
          for (int j = 0; j < NX; j++) sacc += im[OFF_PT + tri(i, j)] * dx[j];
          W.nunew[(size_t)i * SS + o] = sacc;
        }
      }
      if (k < N - 1) {
        double dxn[NX];
#pragma unroll
        for (int i = 0; i < NX; i++) {
          const bool isq = i < NQ;
          double sacc = im[OFF_RC + i];
          sacc += dx[i];
          sacc += (isq ? h : 0.0) * dx[isq ? NQ + i : i];
          sacc += (isq ? h2 : h) * dw[NS + (isq ? i : i - NQ)];
          dxn[i] = sacc;
        }
#pragma unroll
        for (int i = 0; i < NX; i++) dx[i] = dxn[i];
      }
    }
  }
  // = inst_after_recursion on the stored words
  if (!chol_ok) {
    if (usec) {
      if (C::CSCALE && s.theta_c > kCsMin) {   // scaled curvature: the iteration again at half the weight
        W.theta_c[b] = 0.5 * s.theta_c; W.theta_retry[b] = 1; W.redo[b] = 1; W.usedc[b] = 0;
      } else {
        W.redo[b] = 1; W.force_gn[b] = 1; W.usedc[b] = 0;
        if constexpr (C::BACKOFF) {
          const int cb = s.curv_back ? (s.curv_back < kCurvBackMax ? 2 * s.curv_back : kCurvBackMax) : 1;
          W.curv_back[b] = cb; W.curv_skip[b] = cb;
        }
      }
    }
    else W.status[b] = -5;
  } else {
    W.usedc[b] = usec ? 1 : 0;
    W.newstep[b] = 1;
    W.amin_p[b] = (unsigned long long)__double_as_longlong(1.0);
    W.amin_d[b] = (unsigned long long)__double_as_longlong(1.0);
  }
}

// ===========================================================================
// k_step: slack / multiplier steps and step-length partials, stage parallel
// ===========================================================================
// What one lane of the step kernel addresses (same convention as SweepIO).
template <class RP = gdouble>   // RP: where the step lives
struct StepIO {
  const gdouble *zc, *tc, *lc, *grow, *Jq, *gfa;
  const RP *dz;
  size_t SS;
  unsigned loff;
  size_t SSd;       // addressing of dz (see SweepIO)
  unsigned loffd;
};

// ap, ad: fraction-to-the-boundary step lengths of this stage (1 when no row binds); gphi: its merit slope partial
template <class C, class RP = gdouble, class V = RtView>
__device__ __forceinline__ void step_body(const V &v, const StepIO<RP> &io, const int k, const double mu,
                                          double &ap_out, double &ad_out, double &gphi_out) {
  constexpr int NQ = C::NQ, NX = C::NX, NS = C::NS, NV = C::NV;
  const unsigned loff = io.loff;
  const size_t SS = io.SS;
  const gdouble *__restrict__ zc = io.zc;
  const gdouble *__restrict__ tc = io.tc;
  const gdouble *__restrict__ lc = io.lc;
  const gdouble *__restrict__ grow = io.grow;
  const gdouble *__restrict__ Jq = io.Jq;
  double dz[NV], z[NV], gfv[NV];
#pragma unroll
  for (int j = 0; j < NV; j++) {
    dz[j] = io.dz[(size_t)j * io.SSd + io.loffd];
    z[j] = zc[IDXL(j)];
    gfv[j] = io.gfa[IDXL(j)];
  }
  StepRow<C> sr;   // (the row arithmetic: shared with the merged form in sweep_body)
  sr.slope(gfv, dz);
  // Every request of the phase leaves before the first row is evaluated (one wavefront per SIMD hides no latency by
  // itself; left where the arithmetic is, the compiler waits for each small group of loads in turn: a dozen round
  // trips to L2 per call instead of one).  The rows are then evaluated in the old order (the merit slope is a sum).
  struct FkIn { double g, tv, lv, jq[NQ]; };
  auto fk_load = [&](const int r, FkIn &f) __attribute__((always_inline)) {
    const int i = v.fk_row(r), fi = v.fk_idx(r);
    f.g = grow[IDXL(i)]; f.tv = tc[IDXL(i)]; f.lv = lc[IDXL(i)];
#pragma unroll
    for (int a = 0; a < NQ; a++) f.jq[a] = Jq[IDXL(fi * NQ + a)];
  };
  auto fk_row_body = [&](const int r, const FkIn &f) __attribute__((always_inline)) {
    (void)r;
    sr.template fk_row<V>(mu, dz, f.g, f.tv, f.lv, f.jq);
  };
  constexpr int NFKC = []() { if constexpr (V::SPEC) return V::nfkrows() > 0 ? V::nfkrows() : 1; else return 1; }();
  FkIn fkin[NFKC];
  if constexpr (V::SPEC) {
    for_range<0, V::nfkrows()>([&](auto rc) __attribute__((always_inline)) { fk_load(decltype(rc)::value, fkin[decltype(rc)::value]); });
  }
  // single-variable rows, by variable (unconditional clamped requests, see sweep_body), in chunks of VCH variables whose
  // requests leave together: all of them for the small models, one variable at a time for the arms (12 requests per
  // variable: more in flight cost the arm's kernel registers it does not have -- k_step 30 -> 33 us with six)
  constexpr int VCH = NV <= 12 ? NV : 1;
  double tvv[VCH][kVarRows], lvv[VCH][kVarRows], glv[VCH][kVarRows];
  auto chunk_load = [&](auto c0c) __attribute__((always_inline)) {
    constexpr int c0 = decltype(c0c)::value;
#pragma unroll
    for (int jj = 0; jj < VCH; jj++) {
      const int j = c0 + jj < NV ? c0 + jj : NV - 1;
#pragma unroll
      for (int u = 0; u < kVarRows; u++) {
        const int i = v.v_row(j, u);
        const int ii = i >= 0 ? i : 0;
        const bool general = v.v_poff(j, u) >= 0;
        tvv[jj][u] = tc[IDXL(ii)];
        lvv[jj][u] = lc[IDXL(ii)];
        glv[jj][u] = grow[IDXL(general ? ii : 0)];
      }
    }
  };
  auto chunk_rows = [&](auto c0c) __attribute__((always_inline)) {
    constexpr int c0 = decltype(c0c)::value;
#pragma unroll
    for (int jj = 0; jj < VCH; jj++) {
      const int j = c0 + jj;
      if (j >= NV) continue;
#pragma unroll
      for (int u = 0; u < kVarRows; u++) {
        const int i = v.v_row(j, u);
        if (i < 0) continue;
        sr.template var_row<V>(v, k, mu, j, u, z, dz, glv[jj][u], tvv[jj][u], lvv[jj][u]);
      }
    }
  };
  chunk_load(std::integral_constant<int, 0>{});
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (V::SPEC) {
    for_range<0, V::nfkrows()>([&](auto rc) __attribute__((always_inline)) { fk_row_body(decltype(rc)::value, fkin[decltype(rc)::value]); });
  } else {
    // (runtime tables: four rows' requests at a time, clamped to the last row; the row count is uniform)
    const int nfk = v.nfkrows();
    constexpr int FCH = NV <= 12 ? 4 : 1;
    for (int r0 = 0; r0 < nfk; r0 += FCH) {
      FkIn f4[FCH];
#pragma unroll
      for (int u = 0; u < FCH; u++) fk_load(r0 + u < nfk ? r0 + u : nfk - 1, f4[u]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < FCH; u++)
        if (r0 + u < nfk) fk_row_body(r0 + u, f4[u]);
    }
  }
  chunk_rows(std::integral_constant<int, 0>{});
  for_range<1, (NV + VCH - 1) / VCH>([&](auto cc) __attribute__((always_inline)) {
    constexpr int c0 = decltype(cc)::value * VCH;
    chunk_load(std::integral_constant<int, c0>{});
    __builtin_amdgcn_sched_barrier(0);
    chunk_rows(std::integral_constant<int, c0>{});
  });
  ap_out = sr.ap; ad_out = sr.ad; gphi_out = sr.gphi;
}

template <class C, class V>
__global__ __launch_bounds__(kSweepBlock) void k_step(const DevModel M, const DevTables *__restrict__ Tp, const Ws W,
                                              const int B) {
  const int gid = blockIdx.x * kSweepBlock + threadIdx.x;
  const int li = gid % W.Bp;
  const int k = __builtin_amdgcn_readfirstlane(gid / W.Bp);   // (uniform per wavefront, see k_sweep)
  if (li >= *W.n_act || k >= M.N) return;
  const int b = W.act_idx[li];
  if (W.status[b] != ST_ACTIVE || !W.newstep[b]) return;
  (void)B;
  const int cur = W.cur[b];
  StepIO<gdouble> io;
  io.zc = (gdouble *)W.z[cur]; io.tc = (gdouble *)W.t[cur]; io.lc = (gdouble *)W.lam[cur]; io.grow = (gdouble *)W.grow[cur];
  io.Jq = (gdouble *)W.Jq[cur]; io.dz = (gdouble *)W.dz; io.gfa = (gdouble *)W.gfa;
  io.SS = (size_t)M.N * W.Bp;
  io.loff = (unsigned)k * (unsigned)W.Bp + (unsigned)b;
  io.SSd = io.SS; io.loffd = io.loff;
  double ap, ad, gphi;
  const V v(M, *Tp);
  step_body<C, gdouble, V>(v, io, k, W.mu[b], ap, ad, gphi);
  // partial minima -> per-instance step lengths (min is order independent: deterministic)
  atomicMin(&W.amin_p[b], (unsigned long long)__double_as_longlong(ap));
  atomicMin(&W.amin_d[b], (unsigned long long)__double_as_longlong(ad));
  W.gphi[(size_t)k * W.Bp + b] = gphi;
}


// ===========================================================================
// k_fused: whole interior-point iterations of an instance inside ONE wavefront
// ===========================================================================
// The pass kernels above run the batch in lock step: every pass is four launches, every launch streams the
// whole iterate through HBM, and the last few stragglers of a batch cost a full launch chain per iteration.
// Here a wavefront OWNS two instances (32 lanes each, lane = stage) from the first sweep to the converged
// plan: sweep -> reduction (shuffles) -> decisions (registers) -> Riccati recursion (the instance's 32 lanes,
// stage blocks in LDS) -> step lengths (shuffles) -> next sweep, with no kernel boundary, no host look and no
// other wavefront involved.  An instance's state lives in its own contiguous block of the workspace
// ([instance][slot][32 stages]: a half-wavefront moves 256 contiguous bytes per slot), which only its owner
// touches, so it is served by the XCD's L2 / the Infinity Cache; stage records go through LDS (point robot)
// and the per-instance solver words through registers.  Results are bit-identical to the pass kernels: the
// same sweep_body / step_body / inst_decide / riccati_recursion run, and the reductions use the same trees.
// Blocks are independent and of one wavefront: the dispatcher backfills a CU as soon as a pair finishes.
constexpr int kFusedStages = 32;   // stage stride of the per-instance layout = lanes per instance

struct FusedWs {
  double *p;                      // [B][npar][32]
  double *z[2], *t[2], *lam[2], *nu[2];
  double *dz, *nunew, *gfa;
  double *grow[2], *Jq[2];
  double *wlam, *wnu, *wmu;       // [B][m][32], [B][nx][32], [B]: multipliers of the last solve (warm start)
  double *R;                      // [B][N][rs]   (models whose records do not fit LDS)
  double *KP;                     // [B][N][kps]
  int *passes;                    // [0] most passes any instance of the last launch needed, [1] the launch's queue counter
  int *lastp;                     // [B] passes of every instance in the last launch
  int *order;                     // [B] launch order of the next warm-started launch: instances by lastp, longest first
  int *ckey;                      // [B] launch-order keys of a cold launch (k_difficulty)
  long long *stamps;              // [blocks][8] cycles per phase (builds with -DRMPC_STAMPS only; development aid)
  int rs, kps, nv, m, nx, npar, nhs, njqs;
};

// ordering point for data one lane writes to the workspace and another lane of the same wavefront reads later
#define GSYNC()                                              \
  do {                                                       \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
    __builtin_amdgcn_s_waitcnt(0);                           \
    __builtin_amdgcn_wave_barrier();                         \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
  } while (0)

// The phases of the fused kernel are real functions, not inlined bodies: one 500-register function with the sweep,
// the recursion and the step phase inside lets the register allocator spill the loop-carried values of the
// recursion's stage loop to make room for the sweep's straight-line code (measured with the generated views:
// recursion 83 k -> 125 k cycles per pass).  As callees every phase gets the whole register file to itself and the
// few words that live across a call are saved once around it.
#define RMPC_ONE_WAVE   // (occupancy attributes are kernel-only in clang: the phase functions inherit k_fused's, see there)
#define RMPC_PHASE __noinline__ RMPC_ONE_WAVE
template <class C>
__device__ RMPC_PHASE bool fused_recursion_lds(const int N, const double dt, const double mu, const double cw, const int lane,
                                               ldouble *const work, ldouble *const slots, const StepOut<ldouble> so) {
  return riccati_recursion<C, kFusedStages, true, ldouble>(N, dt, mu, cw, lane, work, slots, nullptr, 0, so, slots);
}
template <class C>
__device__ RMPC_PHASE bool fused_recursion_mem(const int N, const double dt, const double mu, const double cw, const int lane,
                                               ldouble *const work, const gdouble *const grec, gdouble *const kpb,
                                               const int kps, const StepOut<gdouble> so) {
  return riccati_recursion<C, kFusedStages, false, gdouble, true>(N, dt, mu, cw, lane, work, grec, kpb, kps, so);
}

// Bases of an instance's block in every array of the fused workspace.  They are recomputed from the instance index
// where a phase needs them (a handful of integer operations) instead of living in registers across the phase calls.
struct FusedPtrs {
  gdouble *pz[2], *pt[2], *pl[2], *pn[2], *pg[2], *pj[2], *pp, *pdz, *pnn, *pgf, *pwl, *pwn;
};
__device__ __forceinline__ FusedPtrs fused_ptrs(const FusedWs &F, size_t b) {
  asm volatile("" : "+v"(b));   // opaque: the bases must not be hoisted out of the pass loop (and spilled there)
  const size_t S = kFusedStages;
  FusedPtrs P;
  P.pz[0] = (gdouble *)F.z[0] + b * F.nv * S; P.pz[1] = (gdouble *)F.z[1] + b * F.nv * S;
  P.pt[0] = (gdouble *)F.t[0] + b * F.m * S; P.pt[1] = (gdouble *)F.t[1] + b * F.m * S;
  P.pl[0] = (gdouble *)F.lam[0] + b * F.m * S; P.pl[1] = (gdouble *)F.lam[1] + b * F.m * S;
  P.pn[0] = (gdouble *)F.nu[0] + b * F.nx * S; P.pn[1] = (gdouble *)F.nu[1] + b * F.nx * S;
  P.pg[0] = (gdouble *)F.grow[0] + b * F.nhs * S; P.pg[1] = (gdouble *)F.grow[1] + b * F.nhs * S;
  P.pj[0] = (gdouble *)F.Jq[0] + b * F.njqs * S; P.pj[1] = (gdouble *)F.Jq[1] + b * F.njqs * S;
  P.pp = (gdouble *)F.p + b * F.npar * S;
  P.pdz = (gdouble *)F.dz + b * F.nv * S;
  P.pnn = (gdouble *)F.nunew + b * F.nx * S;
  P.pgf = (gdouble *)F.gfa + b * F.nv * S;
  P.pwl = (gdouble *)F.wlam + b * F.m * S;
  P.pwn = (gdouble *)F.wnu + b * F.nx * S;
  return P;
}

// The callees of the fused kernel get the pointer block's address as an ordinary (vector register) argument.  Read
// through it as it is, the block came in by eleven vector loads and a full wait before the first useful request of
// the phase, and picking the current / next buffers of an array pair by a run-time index sent the pairs through scratch
// (store, wait, indexed load: a second round trip).  The address is the same in every lane: as a scalar in the constant
// address space the block arrives by scalar loads, and the buffers are picked by selects.
typedef const __attribute__((address_space(4))) FusedWs cFusedWs;
__device__ __forceinline__ cFusedWs *uniform_block(const FusedWs *p) {
  const unsigned long long a = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return (cFusedWs *)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ void load_block(FusedWs &F, const FusedWs *p) {
  static_assert(sizeof(FusedWs) % 8 == 0, "FusedWs is copied in 8-byte words");
  const __attribute__((address_space(4))) unsigned long long *src = (const __attribute__((address_space(4))) unsigned long long *)uniform_block(p);
  unsigned long long *dst = (unsigned long long *)&F;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(FusedWs) / 8); i++) dst[i] = src[i];
}
struct FusedCur {   // an instance's bases with the current / next buffers resolved
  gdouble *zc, *zn, *tc, *tn, *lc, *ln, *nc, *nn, *gc, *gn, *jc, *jn, *pp, *pdz, *pnn, *pgf, *pwl, *pwn;
};
__device__ __forceinline__ FusedCur fused_cur(const FusedWs &F, const size_t b, const int cur) {
  const FusedPtrs P = fused_ptrs(F, b);
  const bool c1 = cur != 0;
  FusedCur Q;
  Q.zc = c1 ? P.pz[1] : P.pz[0]; Q.zn = c1 ? P.pz[0] : P.pz[1];
  Q.tc = c1 ? P.pt[1] : P.pt[0]; Q.tn = c1 ? P.pt[0] : P.pt[1];
  Q.lc = c1 ? P.pl[1] : P.pl[0]; Q.ln = c1 ? P.pl[0] : P.pl[1];
  Q.nc = c1 ? P.pn[1] : P.pn[0]; Q.nn = c1 ? P.pn[0] : P.pn[1];
  Q.gc = c1 ? P.pg[1] : P.pg[0]; Q.gn = c1 ? P.pg[0] : P.pg[1];
  Q.jc = c1 ? P.pj[1] : P.pj[0]; Q.jn = c1 ? P.pj[0] : P.pj[1];
  Q.pp = P.pp; Q.pdz = P.pdz; Q.pnn = P.pnn; Q.pgf = P.pgf; Q.pwl = P.pwl; Q.pwn = P.pwn;
  return Q;
}

// The sweep and the step phase are real functions for the generated views only: with the runtime tables they would
// need the model and the tables through memory instead of through the scalar registers of the kernel.  A call takes
// a handful of scalars -- the callee derives the instance's bases from the pointer block in device memory (scalar
// loads) -- and returns its results by value: with the SweepIO / StepIO structs as arguments and the partials behind
// a reference, the argument and result traffic through scratch was 1.4 KB per lane and pass, more than the 0.9 KB
// the sweep stores by design (round 2, L2 counters: 60 % of the fabric traffic of a launch were writes).
// behind the row tables in device memory: the workspace block, then a copy of the model (rmpc_create)
struct ArmBlock {
  FusedWs F;
  DevModel M;
};
typedef const __attribute__((address_space(4))) ArmBlock cArmBlock;
// The words of a half-wavefront of k_fused that live across the phase calls, parked in LDS beside its solver words
struct FusedHalf {
  double gphi_sum;
  int b, valid, retired, first, ipass, nextslot;
};
// The view a phase FUNCTION reads the problem's structure through: a generated view is a set of constants; the runtime
// tables come through uniform pointers in the constant address space (GView: tables in front of the pointer block,
// the model's copy behind it), i.e. by scalar loads -- round 4: with that the sweep and the step phase of the models
// WITHOUT a generated view (the boxer, the weighted / 2-joint chains) are real functions as well, each with the register
// file to itself, and their requests can leave ahead of the arithmetic (PIPE in sweep_body).
template <class V>
__device__ __forceinline__ V call_view(const FusedWs *Fp) {
  if constexpr (std::is_same<V, GView>::value) {
    const unsigned long long a = (unsigned long long)Fp;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)a), hi = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    const unsigned long long u = ((unsigned long long)hi << 32) | lo;
    typedef const __attribute__((address_space(4))) ArmBlock cArmBlock;
    cArmBlock *const blk = (cArmBlock *)u;
    return GView(&blk->M, (GView::cTables *)(u - sizeof(DevTables)));
  } else {
    return V{};
  }
}
struct StepRes { double ap, ad, gp; };
template <class C, class V, int FIRSTC, bool REC_LDS>
__device__ __noinline__ RMPC_ONE_WAVE Partials fused_sweep_call(const FusedWs *Fp, const int N, const double dt, const int use_curv,
                                                  const size_t b, const int cur, const int k, ldouble *const slots,
                                                  const bool nostep, const double alpha, const double adual, const double mu,
                                                  const int warm) {
  using RP = typename std::conditional<REC_LDS, ldouble, gdouble>::type;
  constexpr int GS = FusedSlots<C>::GS, DZ_OFF = FusedSlots<C>::DZ_OFF, NV = C::NV;
  FusedWs F;
  load_block(F, Fp);   // (scalar loads: uniform address, constant address space)
  const size_t S = kFusedStages;
  const FusedCur Pw = fused_cur(F, b, cur);
  SweepIO<RP> io;
  io.zc = Pw.zc; io.tc = Pw.tc; io.lc = Pw.lc; io.nc = Pw.nc;
  io.zn = Pw.zn; io.tn = Pw.tn; io.ln = Pw.ln; io.nn = Pw.nn;
  io.pp = Pw.pp; io.gro = Pw.gc; io.jqo = Pw.jc; io.grn = Pw.gn; io.jqn = Pw.jn;
  io.gfa = Pw.pgf;
  io.SS = S; io.loff = (unsigned)k; io.kstride = 1u;
  if constexpr (REC_LDS) {
    io.rec = slots + k * GS;
    io.dzp = slots + DZ_OFF; io.nup = slots + DZ_OFF + NV;
    io.SSd = 1; io.loffd = (unsigned)(k * GS); io.kstrided = (unsigned)GS;
  } else {
    io.rec = (gdouble *)F.R + (b * (size_t)N + k) * C::RS;
    io.dzp = Pw.pdz; io.nup = Pw.pnn;
    io.SSd = S; io.loffd = (unsigned)k; io.kstrided = 1u;
  }
  io.wl = Pw.pwl; io.wn = Pw.pwn; io.warm = warm;
  const SweepK sk = {N, dt, use_curv};
  const V v = call_view<V>(Fp);
  Partials q = {0, 0, 0, 0, 0, 0, 0, 0, 1e300, 0};
  sweep_body<C, -1, RP, V, FIRSTC>(sk, v, io, k, FIRSTC != 0, nostep, alpha, adual, mu, q);
  return q;
}
template <class C, class V, bool REC_LDS>
__device__ __noinline__ RMPC_ONE_WAVE StepRes fused_step_call(const FusedWs *Fp, const size_t b, const int cur, const int k,
                                                ldouble *const slots, const double mu) {
  using RP = typename std::conditional<REC_LDS, ldouble, gdouble>::type;
  constexpr int GS = FusedSlots<C>::GS, DZ_OFF = FusedSlots<C>::DZ_OFF;
  FusedWs F;
  load_block(F, Fp);   // (scalar loads: uniform address, constant address space)
  const size_t S = kFusedStages;
  const FusedCur Ps = fused_cur(F, b, cur);
  StepIO<RP> io;
  io.zc = Ps.zc; io.tc = Ps.tc; io.lc = Ps.lc; io.grow = Ps.gc; io.Jq = Ps.jc;
  io.gfa = Ps.pgf;
  io.SS = S; io.loff = (unsigned)k;
  if constexpr (REC_LDS) { io.dz = slots + DZ_OFF; io.SSd = 1; io.loffd = (unsigned)(k * GS); }
  else { io.dz = Ps.pdz; io.SSd = S; io.loffd = (unsigned)k; }
  const V v = call_view<V>(Fp);
  StepRes r = {1.0, 1.0, 0.0};
  step_body<C, RP, V>(v, io, k, mu, r.ap, r.ad, r.gp);
  return r;
}

// Generated views, records in LDS: the step lengths of a fresh step are formed at the beginning of the sweep call
// instead of after the recursion -- the whole wavefront calls (the reductions over the 32
// lanes of the instance run inside), lanes without work skip the bodies.  A pass is two calls: this one and the
// recursion (1.90-1.94 -> 1.97-2.03 M solves/s, same results).  The step lengths and the sweep share one set of
// requests: what both read (slacks, multipliers, row values and gradients, iterate, step) is requested once, at the
// top of the call, and the sweep continues from registers (sweep_body, PHASE 1 / 2).
// What the call hands back, per instance (identical in the 32 lanes of a half: the reductions over the stages run
// inside the call): the reduced partials of the sweep and the step lengths.  Through LDS, not by value -- an
// aggregate of this size is returned in memory, i.e. through scratch: a store, a full wait before the return, and a
// load plus wait in the caller, per pass.
struct SweepStepOut { double f, th, lgs, sumc, badf, rstat, req, rineq, rcomp, minc, amin_p, amin_d, gphi;
#ifdef RMPC_STAMPS
  long long tk[6];
#endif
};
struct SweepStepRes { Partials q; double amin_p, amin_d, gphi; };
template <class C, class V, int FIRSTC>
__device__ __noinline__ RMPC_ONE_WAVE void fused_sweep_step_call(__attribute__((address_space(3))) SweepStepOut *const out,
                                                                 const FusedWs *Fp, const int N, const double dt, const int use_curv,
                                                           const size_t b, const int cur, const int k, ldouble *const slots,
                                                           const bool live, const bool nostep, const bool fresh, const int ls,
                                                           const double amin_p_in, const double amin_d_in, const double gphi_in,
                                                           const double mu, const int warm) {
  constexpr int GS = FusedSlots<C>::GS, DZ_OFF = FusedSlots<C>::DZ_OFF, NV = C::NV;
  FusedWs F;
  load_block(F, Fp);   // (scalar loads: uniform address, constant address space)
  const size_t S = kFusedStages;
  const FusedCur Pw = fused_cur(F, b, cur);
  const V v{};
  SweepIO<ldouble> io;
  io.zc = Pw.zc; io.tc = Pw.tc; io.lc = Pw.lc; io.nc = Pw.nc;
  io.zn = Pw.zn; io.tn = Pw.tn; io.ln = Pw.ln; io.nn = Pw.nn;
  io.pp = Pw.pp; io.gro = Pw.gc; io.jqo = Pw.jc; io.grn = Pw.gn; io.jqn = Pw.jn;
  io.gfa = Pw.pgf;
  io.SS = S; io.loff = (unsigned)k; io.kstride = 1u;
  io.rec = slots + k * GS;
  io.dzp = slots + DZ_OFF; io.nup = slots + DZ_OFF + NV;
  io.SSd = 1; io.loffd = (unsigned)(k * GS); io.kstrided = (unsigned)GS;
  io.wl = Pw.pwl; io.wn = Pw.pwn; io.warm = warm;
  const SweepK sk = {N, dt, use_curv};
  SweepStepRes r;
  const Partials qn = {0, 0, 0, 0, 0, 0, 0, 0, 1e300, 0};
  r.q = qn;
  SecStamps st;   // [0 .. 3] the sections of sweep_body, [4] top loads + step lengths, [5] their reduction
  st.start();
  if constexpr (FIRSTC != 0) {
    // the first pass of a solve takes no step: nothing to merge
    r.amin_p = amin_p_in; r.amin_d = amin_d_in; r.gphi = gphi_in;
    if (live) sweep_body<C, -1, ldouble, V, FIRSTC>(sk, v, io, k, true, nostep, 0.0, 0.0, mu, r.q);
  } else {
    // One set of requests per pass: the top of the sweep (PHASE 1) asks for every word of the stage once and forms
    // the step lengths from the loaded values while the words only the sweep needs are still on their way; the sweep
    // (PHASE 2) continues from the registers.  Every live lane forms the step lengths -- on a pass that is not fresh
    // (line-search retry, null pass) from a step that may be stale -- and `fresh` selects: the two halves of the
    // wavefront may differ in it, and a divergent branch around the requests would serialise them.
    SweepTop<C, V> top;
    StepRow<C> sl;
    if (live) sweep_body<C, -1, ldouble, V, 0, 1>(sk, v, io, k, false, nostep, 0.0, 0.0, mu, r.q, nullptr, &top, &sl);
    double ap = (fresh && live) ? sl.ap : 1.0, ad = (fresh && live) ? sl.ad : 1.0, gp = (fresh && live) ? sl.gphi : 0.0;
    st(4);
    {
      double rs1[1] = {gp}, rm0[1] = {0.0}, rn2[2] = {ap, ad};
      wave_reduce_many<kFusedStages>(rs1, rm0, rn2);
      gp = rs1[0]; ap = rn2[0]; ad = rn2[1];
    }
    st(5);
    r.amin_p = fresh ? fmin(amin_p_in, ap) : amin_p_in;
    r.amin_d = fresh ? fmin(amin_d_in, ad) : amin_d_in;
    r.gphi = fresh ? gp : gphi_in;
    const double alpha = nostep ? 0.0 : ldexp(r.amin_p, -ls), adual = nostep ? 0.0 : r.amin_d;
    if (live) sweep_body<C, -1, ldouble, V, 0, 2>(sk, v, io, k, false, nostep, alpha, adual, mu, r.q, nullptr, &top);
  }
  {
    // (idle lanes and idle halves contribute the neutral elements: their sums are discarded by the caller)
    const Partials &q = r.q;
    double rs5[5] = {q.f, q.th, q.logs, q.sumc, q.bad}, rm4[4] = {q.rstat, q.req, q.rineq, q.rcomp}, rn1[1] = {q.minc};
    wave_reduce_many<kFusedStages>(rs5, rm4, rn1);
    // (every lane of the half stores the same words: no divergence, one LDS request each)
    out->f = rs5[0]; out->th = rs5[1]; out->lgs = rs5[2]; out->sumc = rs5[3]; out->badf = rs5[4];
    out->rstat = rm4[0]; out->req = rm4[1]; out->rineq = rm4[2]; out->rcomp = rm4[3]; out->minc = rn1[0];
    out->amin_p = r.amin_p; out->amin_d = r.amin_d; out->gphi = r.gphi;
    st.get(q, 0, 4);
    if (k == 0) st.put(*out, 0, 6);
  }
}

// (disable_tail_calls: a phase call that hands the callee nothing of the caller's stack gets the `tail` marker, and a
//  function with a tail-marked call site is not eligible for the no-callee-saved-registers optimisation of internal
//  functions: the sweep call then saved and restored 300 registers through scratch on every pass.)
// (amdgpu_waves_per_eu(1, 1): __launch_bounds__' second argument only sets the MINIMUM of waves per SIMD; with the
//  maximum open the instruction scheduler still plans the phase functions -- which inherit the attribute -- for as
//  many waves as it can reach and keeps their register pressure down by serialising the LDS reads of a phase:
//  load, wait, use, load, wait, use.  One wave per SIMD is what the kernel gets anyway: 38 KB of LDS.)
template <class C, bool REC_LDS, class V>
__global__ __launch_bounds__(64, 1) __attribute__((amdgpu_waves_per_eu(1, 1), disable_tail_calls)) void k_fused(const DevModel M, const DevTables *__restrict__ Tp, const FusedWs F, const int B,
                                              const double *__restrict__ xinit, const double *__restrict__ x0,
                                              const double *__restrict__ params, double *__restrict__ zout,
                                              int *__restrict__ exitflag, int *__restrict__ iters_out,
                                              double *__restrict__ kkt, double *__restrict__ obj, const int max_passes,
                                              const int warm_mode, const int use_order, const int save_duals) {
  constexpr int LPI = kFusedStages;
  constexpr int IPW = 2;   // instances per wavefront
  constexpr int NX = C::NX, NV = C::NV;
  using VC = typename std::conditional<V::SPEC, V, GView>::type;   // the view of the phase functions
  // The model and the workspace block are NOT read from the kernel's arguments (M, F: some 90 scalar registers that
  // would live across every phase call, i.e. in lanes of vector registers that go through scratch around the calls),
  // but from their copies behind the row tables (ArmBlock, rmpc_create), through a uniform address in the constant
  // address space: scalar loads at the point of use -- hand-over, the decision's tolerances, the caps.
  auto blk = [&]() __attribute__((always_inline)) -> cArmBlock * {
    unsigned long long a = (unsigned long long)(Tp + 1);
    asm volatile("" : "+s"(a));   // opaque: the loads are not hoisted out of the pass loop
    return (cArmBlock *)a;
  };
  const int half = threadIdx.x / LPI;
  const int k = threadIdx.x & (LPI - 1);       // stage of this lane; also its lane index inside the instance
  // The launch is a queue of instances, not a grid of pairs: a half-wavefront takes instance after instance until the
  // queue is empty (its first one by its position in the grid, the following ones from an atomic counter), so a
  // finished instance never holds its 32 lanes until its partner has finished too, and the grid is no larger than the
  // chip.  In a closed loop (use_order) the queue holds the instances in the order of their previous solve's passes,
  // longest first (k_order): longest-processing-time-first scheduling.  The arithmetic of an instance depends neither
  // on its position in the queue nor on its partner.
  const int N = blk()->M.N;
  const bool stage = k < N;

  // LDS of an instance: the work area of the recursion, and (REC_LDS) its 32 stage slots (FusedSlots)
  constexpr int LW = RicLds<C, LPI>::LDSW;
  constexpr int GS = FusedSlots<C>::GS;
  constexpr int DZ_OFF = FusedSlots<C>::DZ_OFF;
  constexpr int RECW = REC_LDS ? kFusedStages * GS : 0;
  __shared__ double lds[IPW * (LW + RECW)];
  ldouble *const work = (ldouble *)lds + half * (LW + RECW);
  ldouble *const slots = work + LW;

  // ---- per-instance bases of the workspace: computed from the instance index where a phase needs them --------
  const size_t S = kFusedStages;
  // the solver words of the two instances are parked here around the phase calls (the callees own the register file)
  // and beside them the words of the half itself (FusedHalf): nothing of a half lives in registers across a call, where
  // it would be saved to scratch and fetched back with a wait of its own in every pass
  __shared__ Inst sinst[IPW];
  __shared__ FusedHalf shalf[IPW];
  __shared__ SweepStepOut sres[IPW];   // what the sweep call hands back (generated views with LDS records)
  Inst s;
  const bool warm = warm_mode != 0;
  inst_init(s, blk()->M.mu0);
  s.status = 0;                 // (no instance yet)
  int bi = B - 1;               // instance of this half (none: clamped -- addresses stay legal, nothing is written)
  bool valid = false;           // the half holds an instance
  bool retired = false;         // the queue was empty when the half asked: it stays idle
  bool first = true;            // the instance's next pass is its first
  int ipass = 0;                // passes of the instance so far
  int nextslot = blockIdx.x * IPW + half;   // queue position of the half's first instance (-1: ask the counter)
  double gphi_sum = 0.0;   // merit slope of the current step (sum over the stages; step phase)
  // (every lane of an instance holds the same words: its lane 0 parks them, all lanes take them back)
  auto park = [&]() __attribute__((always_inline)) {
    if (k == 0) {
      sinst[half] = s;
      FusedHalf hw;
      hw.gphi_sum = gphi_sum; hw.b = bi; hw.ipass = ipass; hw.nextslot = nextslot;
      hw.valid = valid ? 1 : 0; hw.retired = retired ? 1 : 0; hw.first = first ? 1 : 0;
      shalf[half] = hw;
    }
  };
  // (lane 0's store and the other lanes' loads are ordered by the wavefront fence: without it the compiler may
  //  keep a lane's copy from the previous unpark -- nothing in that lane's own program wrote the words since)
  auto unpark = [&]() __attribute__((always_inline)) {
    WSYNC();
    s = sinst[half];
    const FusedHalf hw = shalf[half];
    gphi_sum = hw.gphi_sum; bi = hw.b; ipass = hw.ipass; nextslot = hw.nextslot;
    valid = hw.valid != 0; retired = hw.retired != 0; first = hw.first != 0;
  };

  PassStamps ps;
  ps.start();
  for (;;) {
    // ---- finished instances leave, idle halves take the next instance of the queue -----------------------------------
    ps.hand_begin();
    {
      const bool over = valid && (s.status == ST_ACTIVE) && ipass >= max_passes;   // deadline (rmpc_set_pass_budget) or cap
      const bool done = valid && (s.status != ST_ACTIVE || over);
      if (__ballot(done || (!valid && !retired)) != 0ull) {
        cArmBlock *const A = blk();
        // The half asks the queue FIRST: the counter's answer travels while the epilogue runs and is looked at behind
        // the epilogue's stores (positions beyond the grid's own; the counter is zeroed before the launch).
        const bool take = (done || !valid) && !retired;   // the half wants the next instance
        bool took = false;
        int qt = 0;
        if (take && nextslot < 0 && k == 0) qt = atomicAdd(A->F.passes + 1, 1);
        if (done) {
          // epilogue: plan in the ABI layout, statistics (the trial point and the step were made visible to the whole
          // wavefront by the ordering points of the pass that ended the solve)
          const size_t b = (size_t)bi;
          const bool c1 = s.cur != 0;
          const bool okd = (s.status == ST_ACTIVE || s.status >= 0) && isfinite(s.mu) && s.mu > 0.0;
          if (stage) {
            const gdouble *zf = (const gdouble *)(c1 ? A->F.z[1] : A->F.z[0]) + b * A->F.nv * S;
            double *zr = zout + (b * N + k) * NV;
            double zv[NV];
#pragma unroll
            for (int j = 0; j < NV; j++) zv[j] = zf[j * S + k];
            if (save_duals) {
              // multipliers for a warm start of the next solve of this instance (a failed solve leaves zeros and mu0):
              // every word of the stage is requested before the first is stored (sets of kDualSet rows: the point
              // robot's 33 rows and 6 costates are one set; slots beyond the last row repeat it -- same address, same
              // value: no tail loop, no branch)
              const int m = A->F.m;
              const gdouble *lf = (const gdouble *)(c1 ? A->F.lam[1] : A->F.lam[0]) + b * m * S;
              const gdouble *nf = (const gdouble *)(c1 ? A->F.nu[1] : A->F.nu[0]) + b * A->F.nx * S;
              gdouble *wl = (gdouble *)A->F.wlam + b * m * S, *wn = (gdouble *)A->F.wnu + b * A->F.nx * S;
              double nv6[NX];
#pragma unroll
              for (int j = 0; j < NX; j++) nv6[j] = nf[j * S + k];
              constexpr int kDualSet = 36;
              for (int i0 = 0; i0 < m; i0 += kDualSet) {
                double lv[kDualSet];
#pragma unroll
                for (int u = 0; u < kDualSet; u++) lv[u] = lf[min(i0 + u, m - 1) * S + k];
                if (i0 == 0) {
#pragma unroll
                  for (int j = 0; j < NV; j++) zr[j] = zv[j];
#pragma unroll
                  for (int j = 0; j < NX; j++) wn[j * S + k] = okd ? nv6[j] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < kDualSet; u++) wl[min(i0 + u, m - 1) * S + k] = okd ? lv[u] : 0.0;
              }
              if (m <= 0) {
#pragma unroll
                for (int j = 0; j < NV; j++) zr[j] = zv[j];
#pragma unroll
                for (int j = 0; j < NX; j++) wn[j * S + k] = okd ? nv6[j] : 0.0;
              }
            } else {
#pragma unroll
              for (int j = 0; j < NV; j++) zr[j] = zv[j];
            }
          }
          if (k == 0) {
            exitflag[b] = (s.status == ST_ACTIVE) ? 0 : s.status;
            iters_out[b] = s.iters;
            kkt[b] = fmax(fmax(s.res_stat, s.res_eq), fmax(s.res_ineq, s.res_comp));
            obj[b] = s.obj;
            if (save_duals) {   // (read by a warm-started launch, k_order_t and rmpc_retarget_device only)
              A->F.wmu[b] = okd ? s.mu : A->M.mu0;
              A->F.lastp[b] = ipass;
            }
            atomicMax(A->F.passes, ipass);
          }
          valid = false;
          s.status = 0;
        }
        if (take) {
          int pos = nextslot;
          if (pos < 0) pos = (int)gridDim.x * IPW + __shfl(qt, half * LPI, 64);
          nextslot = -1;
          if (pos < B) {
            bi = use_order ? A->F.order[pos] : pos;
            const size_t b = (size_t)bi;
            valid = true;
            took = true;
            // prologue: ABI rows of this stage -> the instance's block (x_1 := xinit, mpcModel.py:108).  One set of
            // requests: the stage's row of x0, xinit (lane 0) and every parameter word, then the stores.
            if (stage) {
              gdouble *const pz0 = (gdouble *)A->F.z[0] + b * A->F.nv * S;
              const double *zr = x0 + (b * N + k) * NV;
              double zv[NV];
#pragma unroll
              for (int j = 0; j < NV; j++) zv[j] = zr[j];
              if (k == 0) {
#pragma unroll
                for (int j = 0; j < NX; j++) zv[j] = xinit[b * NX + j];
              }
              if (params) {
                // 16-byte requests from the first 16-byte boundary of the stage's row on (one word in front of it when
                // the row starts between two: odd npar and odd stage index, or a caller's array at an odd word), a
                // last single word when one is left.  Sets of kParSet pairs; slots beyond the row repeat its last pair
                // (same address, same value: no tail loop, no branch).
                const int npar = A->M.npar;
                gdouble *const pp = (gdouble *)A->F.p + b * A->F.npar * S;
                const double *pr = params + (b * N + k) * npar;
                const int head = (int)(((unsigned long long)pr >> 3) & 1ull);
                const int np2 = (npar - head) >> 1;           // whole pairs
                const bool tail = ((npar - head) & 1) != 0;
                const double h0 = head ? pr[0] : 0.0, t0 = tail ? pr[npar - 1] : 0.0;
                const double2 *pq = (const double2 *)(pr + head);
                constexpr int kParSet = 20;
                for (int j0 = 0; j0 < np2; j0 += kParSet) {
                  double2 pv[kParSet];
#pragma unroll
                  for (int u = 0; u < kParSet; u++) pv[u] = pq[min(j0 + u, np2 - 1)];
                  if (j0 == 0) {
#pragma unroll
                    for (int j = 0; j < NV; j++) pz0[j * S + k] = zv[j];
                  }
#pragma unroll
                  for (int u = 0; u < kParSet; u++) {
                    const int j = head + 2 * min(j0 + u, np2 - 1);
                    pp[j * S + k] = pv[u].x; pp[(j + 1) * S + k] = pv[u].y;
                  }
                }
                if (np2 <= 0) {
#pragma unroll
                  for (int j = 0; j < NV; j++) pz0[j * S + k] = zv[j];
                }
                if (head) pp[k] = h0;
                if (tail) pp[(npar - 1) * S + k] = t0;
              } else {
#pragma unroll
                for (int j = 0; j < NV; j++) pz0[j * S + k] = zv[j];
              }
              if constexpr (REC_LDS) {   // the step slots are read (and discarded) by the first sweep: keep them finite
#pragma unroll
                for (int j = 0; j < NV + NX; j++) slots[k * GS + DZ_OFF + j] = 0.0;
              }
            }
            {
              const double mu0 = A->M.mu0;
              inst_init(s, warm ? warm_mu(A->F.wmu[b], mu0) : mu0);
            }
            first = true;
            ipass = 0;
            gphi_sum = 0.0;
          } else {
            retired = true;
            bi = B - 1;
          }
        }
        GSYNC();   // the new instance's block is complete before any lane reads another lane's part
        ps.hand_events(done && k == 0, took && k == 0);
      }
    }
    const bool act = valid && (s.status == ST_ACTIVE);
    ps.hand_end();
    if (__ballot(act) == 0ull) break;   // both halves are idle and the queue is empty
    if (act) ipass++;
    // which copy of the sweep the lane runs this pass (first pass of its instance or not): the two halves of the
    // wavefront may differ (both copies then run, one after the other); an idle half follows its partner
    const bool v1 = act ? first : (__ballot(act && first) != 0ull);
    ps.pass_begin(act && k == 0, v1);
    ps.mark();
    // ---- sweep: trial point, model functions, condensing, stage partials -------------------------------
    Partials q = {0, 0, 0, 0, 0, 0, 0, 0, 1e300, 0};
    // Generated views with LDS records: the step lengths of a fresh step are formed inside the sweep call (MERGE2).
    // (The same reordering for the runtime tables, inline, is bit-identical too and no faster: boxer 0.48 vs 0.50 M.)
    constexpr bool MERGE2 = V::SPEC && REC_LDS;
    park();
    bool fresh = false;
    if constexpr (MERGE2) {
      const bool nostep = first || (s.redo != 0);
      fresh = act && !nostep && (s.newstep != 0);
      const FusedWs *const Fp = (const FusedWs *)(Tp + 1);
      __attribute__((address_space(3))) SweepStepOut *const so = (__attribute__((address_space(3))) SweepStepOut *)&sres[half];
      cArmBlock *const A = blk();
      const double dt = A->M.dt;
      const int use_curv = A->M.use_curv;
      if (v1) fused_sweep_step_call<C, V, 1>(so, Fp, N, dt, use_curv, (size_t)bi, s.cur, k, slots, act && stage, nostep, fresh, s.ls, s.amin_p, s.amin_d, gphi_sum, s.mu, warm ? 1 : 0);
      else fused_sweep_step_call<C, V, 0>(so, Fp, N, dt, use_curv, (size_t)bi, s.cur, k, slots, act && stage, nostep, fresh, s.ls, s.amin_p, s.amin_d, gphi_sum, s.mu, warm ? 1 : 0);
    } else {
      // the sweep is a call (scalars in, partials out): a generated view, or the runtime tables through GView
      if (act && stage) {
        const bool nostep = first || (s.redo != 0);
        double alpha = 0.0, adual = 0.0;
        if (!nostep) {
          alpha = ldexp(s.amin_p, -s.ls);
          adual = s.amin_d;
        }
        const FusedWs *const Fp = (const FusedWs *)(Tp + 1);   // (the pointer block behind the row tables)
        cArmBlock *const A = blk();
        const double dt = A->M.dt;
        const int use_curv = A->M.use_curv;
        if (first) q = fused_sweep_call<C, VC, 1, REC_LDS>(Fp, N, dt, use_curv, (size_t)bi, s.cur, k, slots, nostep, alpha, adual, s.mu, warm ? 1 : 0);
        else q = fused_sweep_call<C, VC, 0, REC_LDS>(Fp, N, dt, use_curv, (size_t)bi, s.cur, k, slots, nostep, alpha, adual, s.mu, warm ? 1 : 0);
      }
    }
    ps.sweep_returned();
    unpark();
    Reduced r;
    if constexpr (MERGE2) {
      // (the call has reduced over the stages and left the instance's words in LDS: unpark's fence orders the reads)
      const SweepStepOut o = sres[half];
      if (fresh) { s.amin_p = o.amin_p; s.amin_d = o.amin_d; gphi_sum = o.gphi; }
      r.f = o.f; r.th = o.th; r.lgs = o.lgs; r.sumc = o.sumc; r.badf = o.badf;
      r.rstat = o.rstat; r.req = o.req; r.rineq = o.rineq; r.rcomp = o.rcomp; r.minc = o.minc;
      ps.sections(sres[half]);
    } else {
      ps.sections(q);
      double rs5[5] = {q.f, q.th, q.logs, q.sumc, q.bad}, rm4[4] = {q.rstat, q.req, q.rineq, q.rcomp}, rn1[1] = {q.minc};
      wave_reduce_many<LPI>(rs5, rm4, rn1);
      r.f = rs5[0]; r.th = rs5[1]; r.lgs = rs5[2]; r.sumc = rs5[3]; r.badf = rs5[4];
      r.rstat = rm4[0]; r.req = rm4[1]; r.rineq = rm4[2]; r.rcomp = rm4[3]; r.minc = rn1[0];
    }
    r.gphi = first ? 0.0 : gphi_sum;
    ps.sweep_reduced();
    GSYNC();   // trial point and records are complete before any lane reads another lane's part
    ps.sweep_end();
    // ---- decisions, then a new step when the trial was accepted --------------------------------------
    bool usec = false;
    bool recurse = false;
    // (the tolerances and caps of the decision: scalar loads from the model's copy behind the row tables)
    if (act) recurse = inst_decide<C>(*(const DevModel *)&blk()->M, s, r, first, usec);
    if (act) first = false;
    ps(PH_DEC);
    park();
    const double mu_r = s.mu;
    const double cw_r = usec ? (C::CSCALE ? s.theta_c : 1.0) : 0.0;   // weight of the curvature terms in this recursion
    bool rec_ok = true;
    if (recurse) {
      bool ok;
      if constexpr (REC_LDS) {
        StepOut<ldouble> so;
        so.dz = slots + DZ_OFF; so.nunew = slots + DZ_OFF + NV; so.SS = 1; so.KS = GS;
        ok = fused_recursion_lds<C>(N, blk()->M.dt, mu_r, cw_r, k, work, slots, so);
      } else {
        cArmBlock *const A = blk();
        const size_t b = (size_t)bi;
        const int kps = A->F.kps;
        StepOut<gdouble> so;
        so.dz = (gdouble *)A->F.dz + b * A->F.nv * S; so.nunew = (gdouble *)A->F.nunew + b * A->F.nx * S; so.SS = S; so.KS = 1;
        ok = fused_recursion_mem<C>(N, A->M.dt, mu_r, cw_r, k, work, (gdouble *)A->F.R + b * (size_t)N * C::RS,
                                    (gdouble *)A->F.KP + b * (size_t)N * kps, kps, so);
      }
      rec_ok = ok;
    }
    unpark();
    if (recurse) inst_after_recursion(s, rec_ok, usec, C::BACKOFF, C::CSCALE);
    GSYNC();   // dz, nunew
    ps(PH_RIC);
    // ---- step lengths of the new step -----------------------------------------------------------------
    // (MERGE2: formed inside the next sweep call -- nothing to park, call or reduce here)
    if constexpr (!MERGE2) {
      double ap = 1.0, ad = 1.0, gp = 0.0;
      const bool stepping = act && (s.status == ST_ACTIVE) && (s.newstep != 0);
      park();
      if (stepping && stage) {
        const FusedWs *const Fp = (const FusedWs *)(Tp + 1);
        const StepRes sr = fused_step_call<C, VC, REC_LDS>(Fp, (size_t)bi, s.cur, k, slots, s.mu);
        ap = sr.ap; ad = sr.ad; gp = sr.gp;
      }
      unpark();
      {
        double rs1[1] = {gp}, rm0[1] = {0.0}, rn2[2] = {ap, ad};
        wave_reduce_many<LPI>(rs1, rm0, rn2);
        gp = rs1[0]; ap = rn2[0]; ad = rn2[1];
      }
      if (stepping) {
        s.amin_p = fmin(s.amin_p, ap);
        s.amin_d = fmin(s.amin_d, ad);
        gphi_sum = gp;
      }
    }
    ps(PH_STEP);
  }
  ps.store(((cArmBlock *)(Tp + 1))->F.stamps, true);
}

#include "rmpc_arm_fused.hpp"   // the arms in one launch (k_fused_arm: a wavefront per instance, a stage per P lanes)

// ===========================================================================
// Scene packing and closed-loop advance: device
// counterparts of the planner's host loops, so that neither the N*npar
// parameter vectors nor the plans have to cross PCIe between control steps.
// ===========================================================================
// Closed loop between two solves: the plant is the model's own ERK2 map applied to the first
// control of the previous plan, the warm start is the shifted plan (shiftHorizon,
// mpcPlanner.py:215-226) or the current state repeated (setX0 "current_state", :228-232).
constexpr int kAdvanceIB = 16;   // instances per block of k_advance
template <class C>
__global__ __launch_bounds__(256) void k_advance(const DevModel M, const double *__restrict__ zprev, double *__restrict__ xinit,
                                                 double *__restrict__ x0, int B, int previous_plan_all,
                                                 const int *__restrict__ exitflag) {
  // A block takes kAdvanceIB instances: one lane each for the plant step, then all 256 lanes shift the plans
  // element by element (contiguous in the ABI layout [b][k][j]: coalesced; one lane per instance walking its
  // N x nvar plan took 76 us for 1024 arms).
  constexpr int NX = C::NX, NS = C::NS, NV = C::NV, IB = kAdvanceIB;
  __shared__ double sx[IB][NX];
  __shared__ int spp[IB];
  const int b0 = blockIdx.x * IB, t = threadIdx.x;
  const int N = M.N;
  if (t < IB && b0 + t < B) {
    const int b = b0 + t;
    double z[NV], xn[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) z[j] = xinit[(size_t)b * NX + j];
#pragma unroll
    for (int j = NX; j < NV; j++) z[j] = zprev[(size_t)b * N * NV + j];  // slack and first control of the plan
    if constexpr (C::ROBOT == RMPC_ROBOT_CHAIN) {
      chain_step<C>(M.dt, z, xn);
    } else {
      double A5[25], B5[10];
      diffdrive_step<C>(M.dt, z, xn, A5, B5, false);
    }
#pragma unroll
    for (int j = 0; j < NX; j++) { xinit[(size_t)b * NX + j] = xn[j]; sx[t][j] = xn[j]; }
    // an instance whose last solve failed (exitflag < 0) has no plan worth shifting: it restarts from its state,
    // as the boxer example of the reference does for its linearisation point (boxer_example.py:194-198)
    spp[t] = (previous_plan_all && !(exitflag && exitflag[b] < 0)) ? 1 : 0;
  }
  __syncthreads();
  const int nb = (B - b0) < IB ? (B - b0) : IB;
  const int per = N * NV;
  for (int e = t; e < nb * per; e += 256) {
    const int ib = e / per, r = e - ib * per, k = r / NV, j = r - k * NV;
    const size_t base = (size_t)(b0 + ib) * per;
    double val;
    if (spp[ib]) val = zprev[base + (size_t)(k + 1 < N ? k + 1 : N - 1) * NV + j];
    else val = j < NX ? sx[ib][j] : 0.0;
    x0[base + r] = val;
  }
  (void)NS;
}

// Steady closed loop (the examples hand the planner a new goal whenever the driver has one,
// setGoalReaching every control step in examples/boxer_example_global.py:203-212): one lane per instance looks at the
// state the plant step has just produced and gives the instance its next goal from its pool when the end link has
// arrived (within tol of the goal) or has dwelt max_dwell control steps on this goal; an instance whose solve FAILED
// (exitflag < 0: infeasible or diverged, a state no plan leads out of) is put back to its start state with a cold
// plan and takes its next goal too.  The goals live in the scene's goal array, so the next parameter packing sees them.
struct RetargetDev {   // rmpc_retarget, device side
  double *xinit, *x0, *goal;
  const int *exitflag, *iters;
  const double *pool, *x_start, *lower, *upper;
  int P;
  int *cursor, *dwell, *failrun;
  double tol, settle_vel;
  int settle_min_dwell, max_dwell, fail_reset_after;
  long long *counts;
  double *wmu;
  double wmu_regoal;
};
template <class C>
__global__ __launch_bounds__(256) void k_retarget(const DevModel M, const DevTables *__restrict__ Tp, int B, const RetargetDev R) {
  constexpr int NQ = C::NQ, NX = C::NX, NV = C::NV;
  const int b = blockIdx.x * 256 + threadIdx.x;
  const bool in = b < B;
  long long *const counts = R.counts;
  // statistics of the control step, summed on the device (no host read inside the loop): exit flags and iterations
  if (counts && R.exitflag) {
    const int ef = in ? R.exitflag[b] : -1000;
    const int it = (in && R.iters) ? R.iters[b] : 0;
    const int cls[4] = {ef == 1, ef == 2, ef == 0, ef < 0 && ef > -1000};
    for (int c = 0; c < 4; c++) {
      const unsigned long long mk = __ballot(cls[c]);
      if ((threadIdx.x & 63) == 0 && mk) atomicAdd((unsigned long long *)&counts[4 + c], (unsigned long long)__popcll(mk));
    }
    int si = it;
    for (int off = 32; off >= 1; off >>= 1) si += __shfl_xor(si, off, 64);
    if ((threadIdx.x & 63) == 0 && si) atomicAdd((unsigned long long *)&counts[8], (unsigned long long)si);
  }
  if (!in) return;
  const RtView v(M, *Tp);
  double *const xi = R.xinit + (size_t)b * NX;
  const bool failed = R.exitflag && R.exitflag[b] < 0;
  // A failed solve (infeasible, diverged, line search): the reference prints the flag and drives on with the action it
  // got (mpcPlanner.py:263-264), its boxer example takes the current pose as the next linearisation point
  // (boxer_example.py:194-198) -- the plant step has applied the returned control, the next solve starts cold from the
  // new state (rmpc_advance_device_flags).  Only an instance that has failed fail_reset_after control steps IN A ROW is
  // put back to its start state (a reset; 0: never).
  int fr = R.failrun ? R.failrun[b] : 0;
  fr = failed ? fr + 1 : 0;
  // ... or one whose configuration has left the joint-limit box by more than a limit row's reach (a robot outside its
  // workspace: the examples' simulator stops a joint at its limit, the plant here is the bare integrator -- a short
  // horizon without a terminal set does overshoot a far goal; counted on its own, counts[12])
  bool oob = false;
  if (R.lower && R.upper) {
    for (int j = 0; j < M.n; j++) {
      const double lo = R.lower[(size_t)b * M.n + j], hi = R.upper[(size_t)b * M.n + j];
      const double margin = 0.05 * (hi - lo);
      oob |= (xi[j] < lo - margin) | (xi[j] > hi + margin);
    }
  }
  const bool reset = oob || (failed && R.fail_reset_after > 0 && fr >= R.fail_reset_after);
  if (counts && oob) atomicAdd((unsigned long long *)&counts[12], 1ull);
  if (reset) {
    for (int j = 0; j < NX; j++) xi[j] = R.x_start[(size_t)b * NX + j];
    for (int k = 0; k < M.N; k++)
      for (int j = 0; j < NV; j++) R.x0[((size_t)b * M.N + k) * NV + j] = j < NX ? R.x_start[(size_t)b * NX + j] : 0.0;
    fr = 0;
  }
  if (R.failrun) R.failrun[b] = fr;
  if (counts && fr > 0) atomicAdd((unsigned long long *)&counts[11], 1ull);
  double q[NQ];
#pragma unroll
  for (int j = 0; j < NQ; j++) q[j] = xi[j];
  Kin<C> kin;
  kin.compute(v, q);
  Vec3 J[NQ];
  const Vec3 pt = kin.template point<0>(v, J);   // slot 0: the goal's end frame (build_tables)
  double *const g = R.goal + (size_t)b * 3;
  const double dx = pt.x - g[0], dy = pt.y - g[1], dz = pt.z - g[2];
  const double dist = sqrt(dx * dx + dy * dy + dz * dz);
  const bool arrived = dist < R.tol;
  // settled: the robot has come to rest on this goal -- with the reference's objective (N w / h on the first row of a
  // module, constraint_avoidance.py:22-31) a goal next to an obstacle is an equilibrium at a distance, not a point reached
  double vmax = 0.0;
  if constexpr (C::ROBOT == RMPC_ROBOT_CHAIN) {
#pragma unroll
    for (int j = 0; j < NQ; j++) vmax = fmax(vmax, fabs(xi[NQ + j]));
  } else {
    vmax = fmax(fabs(xi[6]), fabs(xi[7]));
  }
  int dw = R.dwell[b] + 1;
  const bool settled = !arrived && R.settle_vel > 0.0 && dw >= R.settle_min_dwell && vmax < R.settle_vel;
  const bool late = R.max_dwell > 0 && dw >= R.max_dwell;
  if (arrived || settled || late || reset) {
    const int c = R.cursor[b] + 1;
    R.cursor[b] = c;
    const double *gn = R.pool + ((size_t)b * R.P + (size_t)(c % R.P)) * 3;
    g[0] = gn[0]; g[1] = gn[1]; g[2] = gn[2];
    dw = 0;
    // a new goal moves the optimum: the multipliers of the last solve stay, the barrier parameter of the next solve
    // restarts from mu_regoal (stored so that warm_mu() yields it) instead of 1000 x the converged one
    if (R.wmu && R.wmu_regoal > 0.0 && !failed) R.wmu[b] = R.wmu_regoal;
    if (counts) {
      atomicAdd((unsigned long long *)&counts[reset ? 3 : (arrived ? 0 : (settled ? 1 : 2))], 1ull);
      if (!reset) {
        atomicAdd((unsigned long long *)&counts[9], (unsigned long long)(dist * 1e6));   // distance at the hand-over [um]
        atomicAdd((unsigned long long *)&counts[10], 1ull);
      }
    }
  }
  R.dwell[b] = dw;
}

// Launch order of a COLD fused launch that is larger than the chip (more instances than half-wavefronts: the rest wait
// in the queue).  A lone launch lasts as long as its slowest instance needs from the moment it is dequeued, and the
// slow ones of a cold batch are mostly those that start close to a constraint boundary (the interior-point method's
// first steps are cut by the fraction to the boundary): on the BASELINE scenarios 37-40 of the 40 slowest of 4096
// point robots are in the closer half.  One lane per instance evaluates the distance rows (obstacle, plane, self
// collision) of the start state with the parameters of the second stage and hands k_order_t a key, closest first --
// longest-processing-time-first scheduling with an estimate instead of the previous solve's count.  What an instance
// computes does not depend on its place in the queue (test_launch_order_...).
template <class C>
__global__ __launch_bounds__(64) void k_difficulty(const DevModel M, const DevTables *__restrict__ Tp, const int B,
                                                    const double *__restrict__ xinit, const double *__restrict__ params,
                                                    int *__restrict__ key) {
  constexpr int NQ = C::NQ, NX = C::NX;
  const int b = blockIdx.x * 64 + threadIdx.x;   // (one-wavefront blocks: see k_order_t)
  if (b >= B) return;
  const RtView v(M, *Tp);
  const double *const P = params + ((size_t)b * M.N + (M.N > 1 ? 1 : 0)) * M.npar;
  double q[NQ];
#pragma unroll
  for (int j = 0; j < NQ; j++) q[j] = xinit[(size_t)b * NX + j];
  Kin<C> kin;
  kin.compute(v, q);
  const double rbody = (v.off_r_body() >= 0) ? P[v.off_r_body()] : 0.0;
  double dmin = 1e30, dseg = 1e30;
  // (slot 0 is the goal's end frame when the model has a GoalReaching objective: for its spherical obstacles also the
  //  clearance of the straight segment from the point to the goal -- an instance whose way is blocked takes longer
  //  than one that merely starts next to an obstacle; the sum of the two clearances orders the BASELINE batches
  //  almost as well as the iteration counts themselves: simulated makespans 36 / 60 / 61 / 59 / 102 / 46 iterations
  //  against 35 / 60 / 61 / 59 / 102 / 46 for the true longest-first order and 48 / 72 / 61 / 73 / 102 / 54 by index)
  const bool goal = v.has_goal() != 0;
  Vec3 gv = {0, 0, 0};
  if (goal) gv = {P[v.off_goal()], P[v.off_goal() + 1], P[v.off_goal() + 2]};
  for_range<0, kMaxSlots>([&](auto slc) __attribute__((always_inline)) {
    constexpr int SL = decltype(slc)::value;
    if (SL < v.nslots()) {
      Vec3 J[NQ];
      const Vec3 Pt = kin.template point<SL>(v, J);
      for (int r = v.slot_row_begin(SL); r < v.slot_row_begin(SL + 1); r++) {
        const int kind = v.fk_kind(r), ob = v.fk_obst(r);
        double h;
        if (kind == ROW_RADIAL) {
          const double *o = P + v.off_obst() + 4 * ob;
          const Vec3 dv = {Pt.x - o[0], Pt.y - o[1], Pt.z - o[2]};
          h = sqrt(dot(dv, dv)) - o[3] - rbody;
          if (SL == 0 && goal) {
            const Vec3 sg = {gv.x - Pt.x, gv.y - Pt.y, gv.z - Pt.z}, so = {o[0] - Pt.x, o[1] - Pt.y, o[2] - Pt.z};
            const double l2 = dot(sg, sg);
            double t = l2 > 0.0 ? dot(so, sg) / l2 : 0.0;
            t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
            const Vec3 cv = {so.x - t * sg.x, so.y - t * sg.y, so.z - t * sg.z};
            dseg = fmin(dseg, sqrt(dot(cv, cv)) - o[3] - rbody);
          }
        } else if (kind == ROW_LINEAR) {
          const double *o = P + v.off_lin() + 4 * ob;
          const Vec3 av = {o[0], o[1], o[2]};
          h = fabs(dot(av, Pt) + o[3]) / sqrt(dot(av, av)) - rbody;
        } else {
          h = sqrt(dot(Pt, Pt)) - 2.0 * rbody;
        }
        dmin = fmin(dmin, h);
      }
    }
  });
  // 256 classes of 4 cm of (clearance at the start + clearance of the way), the smallest (and every infeasible start)
  // in the class that is dequeued first
  const double dsum = (dmin > 0.0 ? dmin : 0.0) + (dseg < 1e29 ? (dseg > 0.0 ? dseg : 0.0) : (dmin > 0.0 ? dmin : 0.0));
  const double c = dsum * 25.0;
  key[b] = 255 - (c < 255.0 ? (int)c : 255);
}

}  // namespace rmpc
