// rmpc_sweep.hpp -- the stage-parallel sweep: sweep_body (trial point, rows, condensing, partial sums of one stage),
// what it addresses (SweepIO) and hands back (Partials), and the pass kernel k_sweep.  Part of rmpc_kernels.hip
// (included there, inside namespace rmpc); needs rmpc_solver.hpp.  Includes rmpc_stamps.hpp where the recorders stood.

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
  // single-variable row (j, u) (present: v_row(j, u) >= 0); gl: its stored value (general rows only), or (LIM: the
  // merged call, which does not store it -- ROWWORDS in sweep_body) its limit: the value is formed as the sweep forms it
  template <class V, bool LIM = false, int NV_>
  __device__ __forceinline__ void var_row(const V &v, const int k, const double mu, const int j, const int u, const double (&z)[NV_],
                                          const double (&dz)[NV_], const double gl, const double tv, const double lv) {
    const bool general = v.v_poff(j, u) >= 0;
    double gvv;
    if constexpr (LIM) gvv = (k == 0 && j < C::NX) ? 1.0 : (double)v.v_sgn(j, u) * (z[j] - (general ? gl : v.v_val(j, u)));
    else gvv = general ? gl : ((k == 0 && j < C::NX) ? 1.0 : (double)v.v_sgn(j, u) * (z[j] - v.v_val(j, u)));
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

#include "rmpc_stamps.hpp"   // SecStamps, PassStamps: the cycle-stamp recorders of development builds

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
// MERGED: every later pass of the caller takes its step lengths from PHASE 1, none from step_body (both copies of
// fused_sweep_step_call).
template <class C, int EARLY_MODE = -1, class RP = gdouble, class V = RtView, int FIRSTC = -1, int PHASE = 0, bool MERGED = (PHASE != 0)>
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
  // (ROWWORDS, the scope of ROWSUMS / FINROWS below in the merged call: the value of a general single-variable row --
  //  a limit of q or u from the parameters -- is sg * (z[j] - limit) of the STORED z[j], 1 on the pinned stage.  Its only
  //  reader was the next step-length computation, which here is PHASE 1 of the same call: that asks for the limit instead
  //  of the stored value and forms it as PHASE 2 forms `gold`, the expression that formed the stored word -- one
  //  subtraction and a sign, the same bits, NaN and -0 included -- and neither copy of the call stores it: 12 stores per
  //  stage and pass less, and the 12 lines of `grow` are never fetched.  PHASE 2 asks for the limits again (the line has
  //  just been read): held across the reduction they cost the call 18 registers more than it had.  DESIGN.md 5.1)
  constexpr bool ROWWORDS = MERGED && (C::ROBOT == RMPC_ROBOT_CHAIN) && NQ <= 3 && NS == 0 && V::SPEC && EARLY_MODE < 0;
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
    //  general rows -- ROWWORDS: their limits, ahead of the rest -- are requested for the step lengths alone)
    double gfv[NV], gl[NV][kVarRows];
#pragma unroll
    for (int j = 0; j < NV; j++) {
#pragma unroll
      for (int u = 0; u < kVarRows; u++) {
        gl[j][u] = 0.0;
        if constexpr (ROWWORDS) { if (v.v_row(j, u) >= 0 && v.v_poff(j, u) >= 0) gl[j][u] = P(v.v_poff(j, u)); }
      }
    }
#pragma unroll
    for (int j = 0; j < NV; j++) {
      gfv[j] = gfa[IDXL(j)];
#pragma unroll
      for (int u = 0; u < kVarRows; u++) {
        const int i = v.v_row(j, u);
        if (i < 0) continue;   // (static rows)
        T.vt[j][u] = tc[IDXL(i)];
        T.vl[j][u] = lc[IDXL(i)];
        if constexpr (!ROWWORDS) { if (v.v_poff(j, u) >= 0) gl[j][u] = gro[IDXL(i)]; }
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
        sr.template var_row<V, ROWWORDS>(v, k, mu, j, u, zo, dzo, gl[j][u], T.vt[j][u], T.vl[j][u]);
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
  // (ROWSUMS, the scope of FINROWS below -- the chain without slack in its own order under a generated view: the sums,
  //  maxima and the positivity test over the rows advance at each row.  They are long serial chains whose only use is
  //  `out`, and the compiler ran them all at the end of the stage, with tv, lv and g - tv of every row alive until
  //  then: a third of the later-pass call's register copies.  Same operations in the same order; the defect's terms
  //  are left free, holding them costs registers: DESIGN.md 5.1)
  constexpr bool ROWSUMS = (C::ROBOT == RMPC_ROBOT_CHAIN) && NQ <= 3 && NS == 0 && V::SPEC;
  LaneTests rowbad;
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
    // (cannot happen: fraction to the boundary; keeps the product's sign meaningful.  |=: no branch)
    if constexpr (ROWSUMS) rowbad.add(!(tv > 0.0));
    else bad |= (int)!(tv > 0.0);
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
    if constexpr (ROWSUMS) {
      formed_here(theta); formed_here(lprod); formed_here(lexp); formed_here(rineq); formed_here(rcomp);
      formed_here(sumc); formed_here(minc);
    }
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
      // general rows keep their value for k_step (ROWWORDS: the merged call forms it again, nothing reads the word)
      if constexpr (!ROWWORDS) { if (v.v_poff(j, u) >= 0) grn[IDXL(i)] = g; }
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
        if constexpr (FIN && j >= NQ) finalize_var(std::integral_constant<int, j>{});   // (the first range holds no j < NQ)
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
  // (FINROWS, the chain without slack in its own order under a generated view: a variable j >= NQ is finalised right
  //  behind its rows and the q variables behind the defect as before, where all at the end kept every accumulator alive to
  //  the end of the stage and the merged form paid for that in register copies.  Nothing a variable j >= NQ contributes
  //  to is formed after its rows, and rstat is a maximum: the same values.  Finalising the q variables right behind the
  //  range as well costs the later-pass call 8 accumulation registers more than it had: DESIGN.md 5.1)
  constexpr bool FINROWS = CHAIN && !EARLY && NS == 0 && V::SPEC;
  run_vars(std::integral_constant<int, Ord::NFIRST>{}, std::integral_constant<int, NV>{}, std::integral_constant<bool, FINROWS>{},
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
    } else if constexpr (FINROWS) {
      for_range<0, NQ>(finalize_var);
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
  if constexpr (ROWSUMS) bad |= rowbad.any();
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
