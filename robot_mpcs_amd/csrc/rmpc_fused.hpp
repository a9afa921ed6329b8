// rmpc_fused.hpp -- k_fused: whole interior-point iterations of an instance inside one wavefront, with its workspace
// (FusedWs), its phase functions and the sweep / step calls.  Part of rmpc_kernels.hip (included there, inside namespace
// rmpc); needs rmpc_sweep.hpp, rmpc_inst.hpp, rmpc_riccati.hpp (riccati_recursion, and from rmpc_ric_common.hpp the slots'
// layout FusedSlots, RicLds, StepOut and WSYNC) and rmpc_step.hpp.  rmpc_arm_fused.hpp follows it.

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
  int recurse, usec;   // what the half's decision of this pass said: they wait through the sweep call of an early hand-over
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
    // (MERGED: the later passes of this instance take their step lengths from PHASE 1 below, never from step_body)
    if (live) sweep_body<C, -1, ldouble, V, FIRSTC, 0, true>(sk, v, io, k, true, nostep, 0.0, 0.0, mu, r.q);
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
      // (vector-move exchanges: the caller sends whole halves -- both, or on a pass whose halves differ in the copy they
      //  run the one half of this copy --, and only the bodies above and below are under `live`)
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
    // (idle lanes and idle halves contribute the neutral elements: their sums are discarded by the caller; all 32 lanes
    //  of a half are here, as the vector-move exchanges need)
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
  bool recurse = false;    // the decision of this pass asked for a recursion ...
  bool usec = false;       // ... with the curvature terms
  // (every lane of an instance holds the same words: its lane 0 parks them, all lanes take them back)
  auto park = [&]() __attribute__((always_inline)) {
    if (k == 0) {
      sinst[half] = s;
      FusedHalf hw;
      hw.gphi_sum = gphi_sum; hw.b = bi; hw.ipass = ipass; hw.nextslot = nextslot;
      hw.valid = valid ? 1 : 0; hw.retired = retired ? 1 : 0; hw.first = first ? 1 : 0;
      hw.recurse = recurse ? 1 : 0; hw.usec = usec ? 1 : 0;
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
    recurse = hw.recurse != 0; usec = hw.usec != 0;
  };

  // Generated views with LDS records: the step lengths of a fresh step are formed inside the sweep call (MERGE2).
  // (The same reordering for the runtime tables, inline, is bit-identical too and no faster: boxer 0.48 vs 0.50 M.)
  constexpr bool MERGE2 = V::SPEC && REC_LDS;
  PassStamps ps;
  ps.start();
  for (;;) {
    // A pass of the wavefront is hand-over, sweep, decision -- up to twice -- and then ONE recursion call for both halves.
    // Round 0 is the pass of every half that holds an instance.  A half whose instance stops at that decision would sit
    // out the partner's recursion (half of the pass) and meet its next instance only at the top of the next pass: round 1
    // runs the hand-over for it at once -- epilogue, dequeue, prologue --, then the first sweep and the first decision of
    // the instance it took, so that this instance's first recursion shares the call with the partner's.  The rounds are
    // two trips through one copy of the code (the hand-over is a large part of the kernel's body); an instance keeps its
    // order of sweep, decision, recursion and step, and what a partner does changes nothing in it.
    bool idle = false;
    recurse = false;
    usec = false;
#pragma nounroll
    for (int round = 0;; round = 1) {
      // ---- finished instances leave, idle halves take the next instance of the queue -----------------------------------
      ps.hand_begin();
      bool took = false;
      {
        // deadline (rmpc_set_pass_budget) or cap: looked at at the top of a pass only, behind the instance's recursion
        const bool over = round == 0 && valid && (s.status == ST_ACTIVE) && ipass >= max_passes;
        const bool done = valid && (s.status != ST_ACTIVE || over);
        if (__ballot(done || (!valid && !retired)) != 0ull) {
          cArmBlock *const A = blk();
          // The half asks the queue FIRST: the counter's answer travels while the epilogue runs and is looked at behind
          // the epilogue's stores (positions beyond the grid's own; the counter is zeroed before the launch).
          const bool take = (done || !valid) && !retired;   // the half wants the next instance
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
          ps.hand_events(done && k == 0, took && k == 0, round);
        }
      }
      // who sweeps and decides in this round: every half with an instance; in round 1 the halves that have just taken one
      // (the partner's instance waits between its decision and its recursion)
      const bool act = valid && (s.status == ST_ACTIVE) && (round == 0 || took);
      ps.hand_end();
      if (__ballot(act) == 0ull) {   // round 0: both halves are idle and the queue is empty; round 1: it was empty
        idle = round == 0;
        break;
      }
      if (act) ipass++;
      // which copy of the sweep the lane runs this pass (first pass of its instance or not): the two halves of the
      // wavefront may differ (both copies then run, one after the other); an idle half follows its partner
      const bool v1 = act ? first : (__ballot(act && first) != 0ull);
      ps.pass_begin(act && k == 0, v1, round);
      ps.mark();
      // ---- sweep: trial point, model functions, condensing, stage partials -------------------------------
      Partials q = {0, 0, 0, 0, 0, 0, 0, 0, 1e300, 0};
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
        // (outside `act && stage`: the whole wavefront reduces, idle lanes with the neutral elements)
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
      // (the tolerances and caps of the decision: scalar loads from the model's copy behind the row tables)
      if (act) recurse = inst_decide<C>(*(const DevModel *)&blk()->M, s, r, first, usec);   // (sets both of its half)
      if (act) first = false;
      ps(PH_DEC);
      // Round 1 only for a half that holds an instance this decision has stopped (a retired half holds none).  At most two
      // rounds: an instance that stops at its first decision inside round 1 leaves at the top of the next pass.
      if (round != 0 || __ballot(valid && s.status != ST_ACTIVE) == 0ull) break;
    }
    if (idle) break;
    ps.mark();   // (a round 1 that ended in its hand-over: those cycles are the hand-over's, not the recursion's)
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
      // (an instance that is active here has swept and decided in one of this pass's rounds)
      const bool stepping = valid && (s.status == ST_ACTIVE) && (s.newstep != 0);
      park();
      if (stepping && stage) {
        const FusedWs *const Fp = (const FusedWs *)(Tp + 1);
        const StepRes sr = fused_step_call<C, VC, REC_LDS>(Fp, (size_t)bi, s.cur, k, slots, s.mu);
        ap = sr.ap; ad = sr.ad; gp = sr.gp;
      }
      unpark();
      {
        // (the whole wavefront: lanes that are not stepping bring the neutral elements)
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
