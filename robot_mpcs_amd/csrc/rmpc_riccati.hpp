// rmpc_riccati.hpp -- block-tridiagonal Riccati recursion of one instance, the Riccati step of every kernel family
// (k_riccati, k_fused, k_fused_arm).  Part of rmpc_kernels.hip (included there, inside namespace rmpc, ahead of the
// kernels); needs rmpc_solver.hpp.  Opens with what only the recursion and its callers use (chol_solve, WSYNC, StepOut,
// stage_ptr; the DPP moves dpp_move / dpp_row_bcast are in rmpc_solver.hpp, beside the reductions' exchanges).
//
// riccati_recursion picks one path per model and kernel at compile time; each path is a function of its own:
//   ric_point_robot           fused kernel, chains without slack (n <= 3): Schur form on the LDS slots, with its rollout
//   ric_chain_slack_backward  fused kernel, chains with slack: gain form on the LDS slots       -> ric_rollout
//   ric_dd_backward           fused kernel, diff-drive: records and gains in global memory      -> ric_dd_rollout
//   ric_arm_block             pass and fused arm kernels, n = 5 .. 7 without slack: Schur form + MFMA, with its rollout
//   ric_backward              pass kernels, every other model (generic dense form)               -> ric_rollout
// They share the layout of the instance's LDS row (RicLds) and the per-lane constants of RicCtx.

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

// Completes the LDS requests of the wavefront that are out (s_waitcnt lgkmcnt(0); vmcnt and expcnt stay open: global
// loads in flight are not drained).  For the preheader of a stage loop that takes its first record from requests made
// in front of the loop and every later one from requests made inside it: WSYNC() is a compiler fence and emits no
// instruction, so the requests are still pending at the loop header, and the wait the compiler must then put at the top
// of the stage -- counted for the way in -- on the back edge counts the previous stage's stores instead: LDS operations
// complete in issue order, so every stage waits for stores nobody reads.  With the requests complete before the loop
// is entered the header carries no pending read and the stage's first wait is the one for its own requests.  (The
// builtin, not an asm statement: the compiler's wait insertion sees it and drops the waits it covers.)
__device__ __forceinline__ void lds_requests_done() { __builtin_amdgcn_s_waitcnt(0xC07F); }

// where the recursion leaves the step: dz[slot * SS + k * KS], nunew likewise (pointers advanced to the instance)
template <class RP = gdouble>
struct StepOut {
  RP *dz, *nunew;
  size_t SS, KS;
};

// q[i][j] = v of lane 4 i + j of the reader's row, over the lower triangle from (I, J) on, row by row
template <int I, int J, int NW>
__device__ __forceinline__ void dpp_tri_gather(const double v, double (&q)[NW][NW]) {
  if constexpr (I < NW) {
    q[I][J] = dpp_row_bcast<4 * I + J>(v);
    if constexpr (J < I) dpp_tri_gather<I, J + 1>(v, q);
    else dpp_tri_gather<I + 1, 0>(v, q);
  }
}

// q[j] = v of lane L0 + j of the reader's row, j = J .. NQ - 1
template <int J, int L0, int NQ>
__device__ __forceinline__ void dpp_row_gather(const double v, double (&q)[NQ]) {
  if constexpr (J < NQ) {
    q[J] = dpp_row_bcast<L0 + J>(v);
    dpp_row_gather<J + 1, L0>(v, q);
  }
}

// Address of a per-lane LDS access that moves with the stage: base + k * strb bytes (k uniform, below 2^24).  A lane
// without that access has stride 0 and a word of its own as base: one v_mad_u32_u24, no select.
typedef __attribute__((address_space(3))) char lbyte;
__device__ __forceinline__ ldouble *stage_ptr(ldouble *const base, const unsigned strb, const int k) {
  return (ldouble *)((lbyte *)base + __umul24((unsigned)k, strb));
}

#ifdef RMPC_RIC_STAMPS
// development aid: cycles per phase of the recursion, summed over the wavefronts of all launches
// (static: one copy per translation unit, read through the unit's entries of the variant table)
static __device__ long long g_rst[8];
struct RicStamps {
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
  __device__ __forceinline__ void flush(const int lane) {
    if (lane == 0) {
      for (int i = 0; i < 7; i++) atomicAdd((unsigned long long *)&g_rst[i], (unsigned long long)acc[i]);
      atomicAdd((unsigned long long *)&g_rst[7], 1ull);
    }
  }
};
#else
struct RicStamps {
  __device__ __forceinline__ void start() {}
  __device__ __forceinline__ void operator()(int) {}
  __device__ __forceinline__ void flush(int) {}
};
#endif

template <class C, int LPI>
struct RicLds {
  static constexpr int NX = C::NX, NV = C::NV, NW = C::NW;
  static constexpr int NP2 = NX * (NX + 1) / 2;
  static constexpr int KPW = NW * NX + NW + NP2 + NX + NX;
  // The arms (one wavefront per instance, pass kernels): the chain model uses neither the [A|B] area nor T, and what
  // that saves holds gain images: IMG_SLOTS stages' images stay in LDS between the backward and the forward pass
  // instead of going through the gain record in global memory (budget: a quarter of the CU's 160 KB per wavefront).
  static constexpr bool LIMG = (C::ROBOT == RMPC_ROBOT_CHAIN) && LPI == 64 && NX > 8;
  static constexpr int ABW = LIMG ? 0 : NX * NV;    // [A|B]
  static constexpr int TW = LIMG ? 64 : NX * NV;    // T (chains: only the idle lanes' words)
  // The arms without slack, 9 .. 15 states (n = 5, 6, 7): the Schur-complement path (ric_arm_block) with
  // a work area of its own -- image staging | P / Qxx (NX rows of APS doubles: 8-lane groups of a half wavefront on
  // distinct banks) | [Qux | qu] (NW rows of 16) | Quu (NW rows of 8) | Y operands (8 x 16) | p (16) | dx (2 x 16) |
  // a word per idle lane (64).  The stage records do not pass through LDS there.
  static constexpr bool ARMB = LIMG && C::NS == 0 && NX < 16;
  static constexpr int APS = 24;
  static constexpr int LDSW_ARM = KPW + APS * NX + 16 * NW + 8 * NW + 128 + 16 + 32 + 64;
  static constexpr int LDSW = ARMB ? LDSW_ARM
                                   : KPW + NX * NX + ABW + NV * NV + NV + TW + NX + NX + NW + C::RS;   // doubles per instance
  static constexpr int IMG_SLOTS = LIMG ? (40960 / 8 - LDSW) / KPW : 0;
};

// sum over the 4 lanes of a quad; every lane of the quad ends with the total
__device__ __forceinline__ double dpp_sum4(double v) {
  v += dpp_move<0xB1>(v);    // quad_perm [1, 0, 3, 2]
  v += dpp_move<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  return v;
}
// sum over the 8 aligned consecutive lanes a lane belongs to; every lane of the group ends with the total
__device__ __forceinline__ double dpp_sum8(double v) {
  v += dpp_move<0xB1>(v);    // quad_perm [1, 0, 3, 2]
  v += dpp_move<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  v += dpp_move<0x141>(v);   // row_half_mirror: lane i <-> 7 - i of its 8
  return v;
}

// Fused kernel, small models: everything the recursion exchanges stays in LDS.  An instance owns 32 slots of
// GS doubles, one per stage; slot k holds, in turn, the stage record the sweep wrote ([0, RW]), the gain image
// of the stage that the backward pass leaves for the forward pass ([0, KPW): the record is dead by then), and
// the step of the stage (dz | nu+ at [DZ_OFF, DZ_OFF + NV + NX): behind the record, so that the next sweeps
// read the step while they write their records).
template <class C>
struct FusedSlots {
  static constexpr int KPW = RicLds<C, 32>::KPW;
  static constexpr int DZ_OFF = C::RW + 1;
  static constexpr int NEED = (KPW > DZ_OFF + C::NV + C::NX) ? KPW : DZ_OFF + C::NV + C::NX;
  // 16-byte aligned slots (the sweep stores its record with aligned 16-byte writes) whose stride is NOT a multiple of
  // the 256 bytes the 64 LDS banks span: in the sweep and the step phase lane = stage, i.e. the lanes of an instance
  // address the same word of 32 different slots -- with a stride of 512 bytes every one of those requests was a
  // 32-way bank conflict (SQ_LDS_BANK_CONFLICT: 20 % of the LDS cycles of the kernel)
  // (+2 doubles: a stride of 4 banks -- 16-byte writes of 16 lanes cover the 64 banks once; A/B on one box, four
  //  batches in flight: 2.45-2.52 -> 2.61-2.62 M solves/s)
  static constexpr int GS = (NEED + 7) / 8 * 8 + 2;
};

template <int NX>
__device__ __forceinline__ int ric_tri(const int i, const int j) {   // index of (i, j) in the packed upper triangle
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  return lo * NX - lo * (lo - 1) / 2 + (hi - lo);
}

// What every path starts from: the instance's LDS row (RicLds::LDSW doubles) cut into the image of a stage and the
// work area, the step constants, and the per-lane sources of the dense-block entries in a stage record.
template <class C, int LPI>
struct RicCtx {
  static constexpr int NQ = C::NQ, NX = C::NX, NS = C::NS, NV = C::NV, NW = C::NW;
  static constexpr bool DD = (C::ROBOT == RMPC_ROBOT_DIFFDRIVE);
  // img = [K | kff | P (upper triangle) | p | rc]: what the forward pass needs of a stage, contiguous in
  // LDS so that it leaves for (and returns from) the instance's gain record KP in one request
  static constexpr int NP2 = NX * (NX + 1) / 2;
  static constexpr int KPW = NW * NX + NW + NP2 + NX + NX;
  static constexpr int KPL = (KPW + LPI - 1) / LPI;
  static constexpr int EPL = (NV * NV + LPI - 1) / LPI;   // stage Hessian entries per lane
  static constexpr int TPL = (NX * NV + LPI - 1) / LPI;   // entries of T = P [A|B] (and of [A|B]) per lane
  static constexpr int RPL = (C::RS + LPI - 1) / LPI;     // record entries per lane
  int N, lane;
  double h, h2, mu;
  double cwt;   // weight of the curvature terms (0: Gauss-Newton blocks, 1: exact, 1/2, 1/4: Cfg::CSCALE); Cqq is zero-filled when the model does not use it
  ldouble *img, *sK, *skf, *sPt, *sp, *src, *sP, *sAB, *sQ, *sq, *sT, *sPc, *sdx, *sdw, *srec;   // srec: the stage record as fetched
  // ([A | B] of the holonomic chain is constant, A = [I hI; 0 I], B = [h2 I; h I] on the u columns: every
  //  product with it is written out in closed form and sAB is used by the diff-drive model only)
  // Loop-invariant source of every LDS entry this lane fills: a pointer into the instance's stage
  // records (stage 0; an entry of the record, or its zero slot) plus a constant.  The per-stage fetch
  // is then an unconditional load per entry -- no branch around any load -- and all lanes of the
  // wavefront address the same few cache lines.
  int qp[EPL], cp[EPL];   // record entries a dense-block entry of this lane is made of
  // [A|B] of the diff-drive model: identity outside the reduced (x, y, theta, v, omega) block
  int abp[DD ? TPL : 1];
  double abc[DD ? TPL : 1];

  __device__ __forceinline__ RicCtx(const int N_, const double dt, const double mu_, const double cw, const int lane_,
                                    ldouble *const img_)
      : N(N_), lane(lane_), h(dt), h2(0.5 * dt * dt), mu(mu_), cwt(cw), img(img_) {
    sK = img; skf = sK + NW * NX; sPt = skf + NW; sp = sPt + NP2; src = sp + NX;
    sP = img + KPW; sAB = sP + NX * NX; sQ = sAB + RicLds<C, LPI>::ABW; sq = sQ + NV * NV; sT = sq + NV;
    sPc = sT + RicLds<C, LPI>::TW; sdx = sPc + NX; sdw = sdx + NX; srec = sdw + NW;
#pragma unroll
    for (int u = 0; u < EPL; u++) {
      const int e = lane + LPI * u;
      qp[u] = C::R_ZERO; cp[u] = C::R_ZERO;
      if (e < NV * NV) {
        const int i = e / NV, j = e - i * NV;
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        if (hi < NQ) {
          const int s = lo * NQ - lo * (lo - 1) / 2 + (hi - lo);
          qp[u] = C::R_Q + s;
          if constexpr (C::CURV || C::DDCURV) cp[u] = C::R_C + s;
        } else if (lo == hi) {
          qp[u] = C::R_DG + (lo - NQ);
        } else if (NS > 0 && lo == NX) {
          qp[u] = C::R_CS + hi;
        } else if (NS > 0 && hi == NX) {
          qp[u] = C::R_CS + lo;
        }
        if constexpr (C::DDCURV) {
          // curvature of the unicycle's dynamics outside the q block: variables theta (2), omega (7), u1 | v (6), u0
          auto cls = [](int j) __attribute__((always_inline)) {   // 0 theta, 1 omega, 2 u1, 3 v, 4 u0, -1 none
            return j == 2 ? 0 : (j == 7 ? 1 : (j == NX + NS + 1 ? 2 : (j == 6 ? 3 : (j == NX + NS ? 4 : -1))));
          };
          const int ci = cls(i), cj = cls(j);
          if (ci >= 0 && cj >= 0 && !(ci == 0 && cj == 0)) {
            const int a = ci < cj ? ci : cj, b = ci < cj ? cj : ci;
            // (a, b): alpha-alpha pairs (0,1) (0,2) (1,1) (1,2) (2,2) -> 0 .. 4; alpha-beta pairs (a, 3 + t) -> 5 + 2 a + t
            int idx = -1;
            if (b <= 2) idx = a == 0 ? b - 1 : (a == 1 ? 1 + b : 4);
            else if (a <= 2) idx = 5 + 2 * a + (b - 3);
            if (idx >= 0) cp[u] = C::R_D + idx;
          }
        }
      }
    }
    if constexpr (DD) {
#pragma unroll
      for (int u = 0; u < TPL; u++) {
        const int e = lane + LPI * u;
        abp[u] = C::R_ZERO; abc[u] = 0.0;
        if (e < NX * NV) {
          const int i = e / NV, j = e - i * NV;
          const int ri = (i < 3) ? i : (i >= 6 ? i - 3 : -1);
          if (j < NX) {
            const int rj = (j < 3) ? j : (j >= 6 ? j - 3 : -1);
            if (ri >= 0 && rj >= 0) abp[u] = C::R_A5 + (ri * 5 + rj);
            else abc[u] = (i == j) ? 1.0 : 0.0;
          } else if (j >= NX + NS && ri >= 0) {
            abp[u] = C::R_B5 + (ri * 2 + (j - NX - NS));
          }
        }
      }
    }
  }
};

// ---- fused kernel, holonomic chain without slack, n <= 3 (the point robot): Schur-complement form on the slots --------
// Round 4.  At four wavefronts per CU the recursion of k_fused is bound by the LDS: the gain form below
// (ric_chain_slack_backward, kept for the chains with the slack variable) reads 78 doubles per lane and backward stage
// and 24 per forward stage; this one reads 37 and 17 -- the block form of the arms' path (ric_arm_block) at
// half-wavefront width:
//   A  lane (i, j) of an n x n grid (lane 4 i + j: a quad per row of the grid, all of it in the first 16-lane row of the
//      instance) reads S, T, T', V of the cost-to-go once and forms the seven block entries of [A|B]^T P [A|B]; its eight
//      record entries come from the stage's slot one stage ahead; g = P rc + p by DPP sums over the quad, lanes
//      j = 0, 1, 2 finish the gradient entries q_i, v_i, u_i;
//   B  Cholesky of Quu in every lane of the first row -- its entries come straight from phase A's registers by DPP row
//      broadcast, so the factorisation runs while [Qux | qu] goes through LDS --, Y = L^-1 [Qux | qu] (a column per
//      lane), the gains K = -L^-T Y behind it;
//   C  [P | p] = [Qxx | qx] - Y^T [Y | y]: an entry per lane and turn, (i, j) and (j, i) the same products in the
//      same order (Qxx is formed symmetrically): symmetric without the 0.5 (a + a^T) of the gain form.
// The rollout forms dw, nu+ and dx+ from dx alone with one role per lane (one row of the image per lane); dx goes from
// lane to lane by DPP row moves, not through LDS.
template <class C, int LPI>
__device__ __forceinline__ bool ric_point_robot(const RicCtx<C, LPI> &ctx, ldouble *const slots, const StepOut<ldouble> so) {
  constexpr int NQ = C::NQ, NX = C::NX, NW = C::NW, NP2 = RicCtx<C, LPI>::NP2, GS = FusedSlots<C>::GS;
  // (the horizon is the same in every lane: as a scalar, the stage loops count and branch in scalar registers)
  const int N = __builtin_amdgcn_readfirstlane(ctx.N), lane = ctx.lane;
  const double h = ctx.h, h2 = ctx.h2, mu = ctx.mu, cwt = ctx.cwt;
  ldouble *const img = ctx.img;
  bool chol_ok = true;
  constexpr int n = NQ;
  constexpr int OFF_KFF = NW * NX, OFF_PT = OFF_KFF + NW, OFF_P = OFF_PT + NP2, OFF_RC = OFF_P + NX;
  constexpr unsigned SB = GS * 8;   // bytes from a slot to the next
  static_assert(LPI == 32 && NW == n && NX == 2 * n && NX + 1 <= 8, "point-robot path: holonomic chain without slack, n <= 3");
  static_assert(20 * NW + 16 + 4 + 32 + NX <= RicLds<C, LPI>::LDSW, "point-robot path: work area");
  // work area: [Qux | qu] (NW rows of 8) | 4 NW words, the first of them the factorisation's flag | Y (NW rows of 8) |
  // 16 words without a use (dx of the rollout, before it stayed in registers: the layout is kept) | four zeros | a word
  // per idle lane (and NX behind them: an idle lane's stores go to its word plus the offset the busy lanes use)
  ldouble *const aQux = img, *const aQuu = aQux + 8 * NW, *const aY = aQuu + 4 * NW, *const adx = aY + 8 * NW,
               *const azero = adx + 16, *const adum = azero + 4;
  ldouble *const dummy = adum + lane;
  // -- lane (gi, gj), block position (ii, jj): the lane keeps its entries S, T, T', V of the cost-to-go (and p_i in
  //    lanes gj = 0, p_{n+i} in lanes gj = 1) in registers from stage to stage -----------------------------------------
  static_assert(4 * NW <= 16 && NX + 1 <= 16, "point-robot path: block grid and gain columns in one 16-lane row");
  const int gi = lane >> 2, gj = lane & 3;
  const bool gval = gi < n, gon = gval && gj < n;
  const int ii = gval ? gi : 0, jj = gj < n ? gj : 0;
  const bool gdiag = gon && ii == jj;
  const int qlo = ii < jj ? ii : jj, qhi = ii < jj ? jj : ii;
  const int tq = qlo * n - qlo * (qlo - 1) / 2 + (qhi - qlo);
  const int jme = gj == 0 ? ii : (gj == 1 ? n + ii : (gj == 2 ? 2 * n + ii : 0));   // gradient entry of lanes gj <= 2
  const double gc1 = gj == 0 ? 1.0 : (gj == 1 ? h : h2), gc2 = gj == 0 ? 0.0 : (gj == 1 ? 1.0 : h);
  // Record entries of this lane, as four pairs at a fixed distance: (Q, C) at tq, the diagonal entries (DG_i, DG_{n+i}),
  // the defect (rc_j, rc_{n+j}), (q0, q1) at jme.  Every access of the stage loops is base + k * stride with a per-lane
  // base and stride set here, once: a lane whose block position takes no diagonal entry, or no defect entry, reads the
  // zeros of the work area with stride 0 -- the same 0.0 into the same operation as a select would give, without the
  // select -- and a lane without a store writes to its dummy word with stride 0.
  static_assert(n + 1 <= 4, "point-robot path: zeros of the work area");
  constexpr int DQC = C::R_C - C::R_Q, DQ01 = C::R_Q1 - C::R_Q0;
  ldouble *const rQ = slots + C::R_Q + tq, *const rG = slots + C::R_Q0 + jme;
  ldouble *const rD = gdiag ? slots + C::R_DG + ii : azero, *const rR = gj < n ? slots + C::R_RC + jj : azero;
  const unsigned strD = gdiag ? SB : 0u, strR = gj < n ? SB : 0u;
  unsigned strU = SB;   // (every lane: kept in a vector register like the others, so that these addresses are one multiply-add too)
  asm volatile("" : "+v"(strU));
  ldouble *const dUq = gon ? aQux + ii * 8 + jj : dummy, *const dUv = gon ? aQux + ii * 8 + n + jj : dummy;
  ldouble *const dqu = (gval && gj == 2) ? aQux + ii * 8 + NX : dummy;   // gradient of u_i (q_i, v_i stay in registers)
  const bool rcw = lane < n;   // lanes (0, jj) put the defect of the stage into the image
  ldouble *const wRC = rcw ? slots + OFF_RC + lane : dummy;
  const unsigned strRC = rcw ? SB : 0u;
  const int myrow = gj == 1 ? n + ii : ii;   // row of [P | p] whose p entry this lane forms (lanes gj = 0, 1)
  // where the lane's entries of the new cost-to-go go in the image of the stage (packed upper triangle; p)
  const bool wST = gon && ii <= jj, wp = gval && gj <= 1;
  ldouble *const wS = wST ? slots + OFF_PT + ric_tri<NX>(ii, jj) : dummy, *const wT = gon ? slots + OFF_PT + ric_tri<NX>(ii, n + jj) : dummy,
               *const wV = wST ? slots + OFF_PT + ric_tri<NX>(n + ii, n + jj) : dummy, *const wP = wp ? slots + OFF_P + myrow : dummy;
  const unsigned strST = wST ? SB : 0u, strT = gon ? SB : 0u, strP = wp ? SB : 0u;
  // -- phase B: gain column of this lane (NX: the gradient column) ---------------------------------------------------
  const int bc = lane <= NX ? lane : 0;
  ldouble *const dY = lane <= NX ? aY + bc : dummy;
  const int ystr = lane <= NX ? 8 : 0;
  const int koff = lane < NX ? lane : OFF_KFF, kstr = lane < NX ? NX : (lane == NX ? 1 : 0);
  ldouble *wK[NW];   // the lane's column of K (lanes < NX: entries NX apart), kff (lane NX: consecutive)
#pragma unroll
  for (int i = 0; i < NW; i++) wK[i] = lane <= NX ? slots + koff + i * kstr : dummy;
  const unsigned strK = lane <= NX ? SB : 0u;
  if (lane < 4) azero[lane] = 0.0;
  WSYNC();
  double rn[8];   // record of the stage at hand; the next stage's is requested into it once phase A has used it
  rn[0] = stage_ptr(rQ, strU, (N - 1))[0]; rn[1] = stage_ptr(rQ, strU, (N - 1))[DQC];
  rn[2] = stage_ptr(rD, strD, N - 1)[0]; rn[3] = stage_ptr(rD, strD, N - 1)[n];
  rn[4] = stage_ptr(rR, strR, N - 1)[0]; rn[5] = stage_ptr(rR, strR, N - 1)[n];
  rn[6] = stage_ptr(rG, strU, (N - 1))[0]; rn[7] = stage_ptr(rG, strU, (N - 1))[DQ01];
  double S = 0.0, T = 0.0, U = 0.0, V = 0.0, p1 = 0.0, p2 = 0.0;   // P = 0, p = 0 behind the last stage
  WSYNC();
  lds_requests_done();   // (the record of stage N - 1 is in: no stage waits at its top)
  RicStamps rst;
  rst.start();
  for (int k = N - 1; k >= 0; k--) {
    // (slot k: the record of stage k, in registers by now; becomes its image)
    // ---- phase A: the blocks of [A|B]^T P [A|B] at (ii, jj); Qxx stays in registers --------------------------------
    const double rcj = rn[4], rcnj = rn[5];   // (0.0 in the lanes gj >= n)
    const double tv = h * S + T, tu = h2 * S + h * T, bv = h * U + V, bu = h2 * U + h * V;
    const double qq = S + (rn[0] - cwt * rn[1]);
    const double vq = h * S + U;
    double vv = (h * (h * S + (T + U)) + V) + rn[2];   // (the diagonal entries: 0.0 off the diagonal)
    asm volatile("" : "+v"(vv));   // formed here, not where phase C takes it: the record's registers are free for the next stage's
    const double uq = h2 * S + h * U, uv = h2 * tv + h * bv;
    const double uu = (h2 * tu + h * bu) + rn[3];
    *dUq = uq; *dUv = uv;   // (Quu stays in registers: phase B takes it by row broadcast)
    // g = P rc + p: the group's partial products, summed over its lanes (gj < n <= 3: one quad)
    const double g1 = p1 + dpp_sum4(S * rcj + T * rcnj), g2 = p2 + dpp_sum4(U * rcj + V * rcnj);
    const double gme = (rn[6] - mu * rn[7]) + (gc1 * g1 + gc2 * g2);   // gradient entry q_i / v_i / u_i (gj = 0, 1, 2)
    *dqu = gme;
    {
      ldouble *const w = stage_ptr(wRC, strRC, k);
      w[0] = rn[4]; w[n] = rn[5];
    }
    WSYNC();
    rst(1);
    // ---- phase B: Cholesky of Quu (every lane), Y = L^-1 [Qux | qu] (one column per lane) ------------------------------
    {
      double qw[NW][NW], colv[NW];
#pragma unroll
      for (int i = 0; i < NW; i++) colv[i] = aQux[i * 8 + bc];
      __builtin_amdgcn_sched_barrier(0);
      // The record of the next stage (stage k - 1) is requested here: phase A, above the scheduling barrier, has taken
      // every entry of this stage's, so it arrives in the same registers -- no copy from a prefetch buffer -- behind the
      // operands of the factorisation and long before the next phase A.  (Stage 0 requests its own slot again and
      // nobody takes the answer.)
      {
        const int kn = k > 0 ? k - 1 : 0;
        rn[0] = stage_ptr(rQ, strU, kn)[0]; rn[1] = stage_ptr(rQ, strU, kn)[DQC];
        rn[2] = stage_ptr(rD, strD, kn)[0]; rn[3] = stage_ptr(rD, strD, kn)[n];
        rn[4] = stage_ptr(rR, strR, kn)[0]; rn[5] = stage_ptr(rR, strR, kn)[n];
        rn[6] = stage_ptr(rG, strU, kn)[0]; rn[7] = stage_ptr(rG, strU, kn)[DQ01];
      }
      __builtin_amdgcn_sched_barrier(0);   // (every read of the phase is out before the chain of the factorisation begins)
      // Quu (lower triangle) from the lanes 4 i + j that formed it in phase A: vector moves, no LDS, so the factorisation
      // starts here and the wait for [Qux | qu] stands behind it, before the forward substitution.  Only the first row of
      // the instance holds Quu: the other lanes factor what their own row hands them, into their dummy words.
      dpp_tri_gather<0, 0>(uu, qw);
      double L[NW][NW], invd[NW];
#pragma unroll
      for (int j = 0; j < NW; j++) {
        double dg = qw[j][j];
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
          double sacc = qw[i][j];
#pragma unroll
          for (int l = 0; l < j; l++) sacc -= L[i][l] * L[j][l];
          L[i][j] = sacc * inv;
        }
      }
      double y[NW];
#pragma unroll
      for (int i = 0; i < NW; i++) {
        double sacc = colv[i];
#pragma unroll
        for (int l = 0; l < i; l++) sacc -= L[i][l] * y[l];
        y[i] = sacc * invd[i];
        dY[i * ystr] = y[i];
      }
      WSYNC();
      rst(3);
      // ---- phase C: [P | p] = [Qxx | qx] - Y^T [Y | y] at the lane's own block position: the next stage's phase A
      //      starts from registers (no store of P, no ordering point, no read-back) ---------------------------------------
      double yiq[NW], yiv[NW], yjq[NW], yjv[NW], yg[NW];
#pragma unroll
      for (int l = 0; l < NW; l++) {
        yiq[l] = aY[l * 8 + ii]; yiv[l] = aY[l * 8 + n + ii]; yjq[l] = aY[l * 8 + jj]; yjv[l] = aY[l * 8 + n + jj];
        yg[l] = aY[l * 8 + NX];
      }
      __builtin_amdgcn_sched_barrier(0);
      // (while the operands arrive: the gains K = -L^-T Y of this lane's column, for the rollout only)
      double x[NW];
#pragma unroll
      for (int i = NW - 1; i >= 0; i--) {
        double sacc = y[i];
#pragma unroll
        for (int l = i + 1; l < NW; l++) sacc -= L[l][i] * x[l];
        x[i] = sacc * invd[i];
      }
#pragma unroll
      for (int i = 0; i < NW; i++) *stage_ptr(wK[i], strK, k) = -x[i];
      double sn = qq, tn_ = tv, un = vq, vn = vv, pn = gme;
#pragma unroll
      for (int l = 0; l < NW; l++) {
        sn -= yiq[l] * yjq[l]; tn_ -= yiq[l] * yjv[l]; un -= yiv[l] * yjq[l]; vn -= yiv[l] * yjv[l];
        pn -= (gj == 1 ? yiv[l] : yiq[l]) * yg[l];
      }
      S = sn; T = tn_; U = un; V = vn;
      p1 = dpp_move<0x00>(pn);   // quad_perm [0, 0, 0, 0]: p_i from lane gj = 0 of the quad
      p2 = dpp_move<0x55>(pn);   // quad_perm [1, 1, 1, 1]: p_{n+i} from lane gj = 1
      *stage_ptr(wS, strST, k) = sn;
      *stage_ptr(wT, strT, k) = tn_;
      *stage_ptr(wV, strST, k) = vn;
      *stage_ptr(wP, strP, k) = pn;
    }
    rst(4);
  }
  // the flag of the first row (its lanes agree: the same Quu) for all lanes of the instance, once, through a word of the
  // work area and the ordering point that ends the loop anyway
  *(lane == 0 ? aQuu : dummy) = chol_ok ? 1.0 : 0.0;
  WSYNC();
  chol_ok = aQuu[0] != 0.0;
  if (!chol_ok) return false;
  // ---- rollout: dw = kff + K dx, nu+ = p + P dx, dx+ = rc + [A|B][dx; dw]: dx stays in registers, no ordering point -------
  const bool fA = lane < NW, fB = lane >= NW && lane < NW + NX, fC = lane >= NW + NX && lane < NW + 2 * NX;
  const int fi = fA ? lane : (fB ? lane - NW : (fC ? lane - NW - NX : 0));   // entry of dw / nu+ / dx+
  const int fw = fC ? (fi < n ? fi : fi - n) : fi;                             // the entry of dw a dx+ lane needs
  // (every lane reads a row of the image, idle lanes that of lane 0: the image addresses are slot + a per-lane constant)
  const ldouble *const imoff = slots + (fB ? OFF_P + fi : OFF_KFF + fw), *const imrc = slots + OFF_RC + fi;
  const ldouble *imrow[NX];
#pragma unroll
  for (int j = 0; j < NX; j++) imrow[j] = slots + (fB ? OFF_PT + ric_tri<NX>(fi, j) : fw * NX + j);
  const bool fpos = fC && fi < n;   // a position lane of dx+: it takes the velocity entry n lanes up
  const double fca = fi < n ? h : 0.0, fcb = fi < n ? h2 : h;
  // the lane's store, one per stage: dz (dw of lanes fA, dx of lanes fC) or nu+ (lanes fB; none at stage 0: x_0 is given)
  ldouble *const wst0 = (fA || fC) ? so.dz + (fA ? NX + lane : fi) : dummy, *const wst = fB ? so.nunew + fi : wst0;
  const unsigned strst0 = (fA || fC) ? SB : 0u, strst = fB ? SB : strst0;
  // dx lives in the registers of the lanes that form it: lane NW + NX + j holds entry j (`dxme`; the other lanes carry a
  // finite word nobody takes).  A stage hands it round by DPP row moves -- every lane takes the NX entries by
  // row_newbcast (dpp_row_bcast: one v_mov_b64_dpp each), a position lane its velocity by row_shl:n, made in every lane
  // and selected afterwards (inside a branch the source lanes would sit the move out) -- where it used to be stored to
  // the work area, ordered and read back: no store of dx, no ordering point in the stage, no LDS read that waits on
  // the previous stage.  All of it is in the first 16-lane row of the instance, and whole halves are here (the flag
  // above is the instance's).  The lane's row of the image does not depend on dx: it is requested a stage ahead into
  // the other of two register sets (`ra` / `rb`: NX entries of the row, the offset kff / p, the defect), so a stage
  // waits for no LDS answer it has just asked for.  The image of a stage is read a stage before its step is stored over
  // it (same wavefront: DS instructions execute in issue order).  Same operations on the same values in the same order
  // as the exchange through LDS; the first dx is zero.
  // (dx through the crossbar -- ds_bpermute, 16 crossbar instructions per stage -- was measured slower than the store and
  //  read-back: 2.85 -> 2.75 M solves/s on cfg2 with four batches in flight; the row moves are vector moves: DESIGN.md 5.1)
  static_assert(NW + 2 * NX <= 16, "point-robot path: the rollout's lanes in one 16-lane row");
  constexpr int FC0 = NW + NX;   // lane of dx_0
  auto request = [&](double (&r)[NX + 2], const int k) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NX; j++) r[j] = imrow[j][k * GS];
    r[NX] = imoff[k * GS];
    r[NX + 1] = imrc[k * GS];
  };
  double dxme = 0.0;
  // One stage on the image in `cur`; the image of stage kn is requested into `nxt` first (`pf`; the last stage asks for
  // nothing).  The stage loop runs two stages per turn, so that the two register sets change roles without a copy and
  // the requests of a turn are one set of addresses plus constants.
  auto fwd = [&](const int k, const double (&cur)[NX + 2], double (&nxt)[NX + 2], const int kn, const bool pf,
                 const bool first) __attribute__((always_inline)) {
    if (pf) request(nxt, kn);
    __builtin_amdgcn_sched_barrier(0);   // (the requests leave before the chain of the stage begins)
    double dxv[NX];
    dpp_row_gather<0, FC0>(dxme, dxv);
    const double dsh = dpp_move<0x100 + n>(dxme);   // row_shl:n
    const double d0 = dxme, d1 = fpos ? dsh : dxme;
    double sacc = cur[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) sacc += cur[j] * dxv[j];
    *stage_ptr(first ? wst0 : wst, first ? strst0 : strst, k) = fC ? d0 : sacc;
    double sx = cur[NX + 1];
    sx += d0;
    sx += fca * d1;
    sx += fcb * sacc;
    dxme = sx;   // (the last stage's dx+ is formed like every other: nobody takes it)
    rst(6);
  };
  double ra[NX + 2], rb[NX + 2];
  request(ra, 0);
  fwd(0, ra, rb, N > 1 ? 1 : 0, true, true);
  int k = 1;
  for (; k + 2 < N; k += 2) {
    fwd(k, rb, ra, k + 1, true, false);
    fwd(k + 1, ra, rb, k + 2, true, false);
  }
  // (behind the pairs: one stage or two, the last one without a request)
  if (k < N) {
    const bool two = k + 1 < N;
    fwd(k, rb, ra, two ? k + 1 : k, true, false);
    if (two) fwd(k + 1, ra, rb, 0, false, false);
  }
  rst.flush(lane);
  return true;
}

// ---- fused kernel, holonomic chain: the backward pass on the instance's LDS slots ---------------------
// Same arithmetic per entry as the generic path below, organised for a wavefront that runs alone on its
// SIMD: the record is read where the sweep left it (slot k), the image of the stage is written where the
// forward pass will read it (slot k: the record is dead by then), every phase issues all its LDS reads
// before the first use (one wait per phase instead of one per entry), nothing is predicated except the
// stores, and the cost-to-go products of a lane's q entry are formed by the lane itself instead of going
// through another LDS exchange: three waits per stage instead of about twenty.
template <class C, int LPI>
__device__ __forceinline__ bool ric_chain_slack_backward(const RicCtx<C, LPI> &ctx, ldouble *const slots, RicStamps &rst) {
  constexpr int NQ = C::NQ, NX = C::NX, NS = C::NS, NV = C::NV, NW = C::NW, GS = FusedSlots<C>::GS;
  constexpr int NP2 = RicCtx<C, LPI>::NP2, EPL = RicCtx<C, LPI>::EPL;
  const int N = ctx.N, lane = ctx.lane;
  const double h = ctx.h, h2 = ctx.h2, mu = ctx.mu, cwt = ctx.cwt;
  ldouble *const sP = ctx.sP, *const sp = ctx.sp, *const sQ = ctx.sQ, *const sq = ctx.sq, *const srec = ctx.srec;
  const int (&qp)[EPL] = ctx.qp, (&cp)[EPL] = ctx.cp;
  bool chol_ok = true;
  constexpr int OFF_KFF = NW * NX, OFF_PT = NW * NX + NW, OFF_P = OFF_PT + NP2, OFF_RC = OFF_P + NX;
  // loop-invariant per-lane constants of the Q entries (sum_{a,b} l_a c_b P_ab, see the generic path)
  int o11[EPL];
  double l1[EPL], l2[EPL], c1[EPL], c2[EPL];
  bool qok[EPL];
#pragma unroll
  for (int u = 0; u < EPL; u++) {
    const int e = lane + LPI * u;
    qok[u] = e < NV * NV;
    const int ec = qok[u] ? e : 0;
    const int i = ec / NV, j = ec - i * NV;
    const int ki = i < NQ ? 0 : (i < NX ? 1 : (i >= NX + NS ? 2 : 3));
    const int kj = j < NQ ? 0 : (j < NX ? 1 : (j >= NX + NS ? 2 : 3));
    const bool on = ki != 3 && kj != 3;
    const int ii = !on ? 0 : (ki == 0 ? i : (ki == 1 ? i - NQ : i - NX - NS));
    const int jj = !on ? 0 : (kj == 0 ? j : (kj == 1 ? j - NQ : j - NX - NS));
    o11[u] = ii * NX + jj;
    l1[u] = !on ? 0.0 : (ki == 0 ? 1.0 : (ki == 1 ? h : h2)); l2[u] = !on ? 0.0 : (ki == 0 ? 0.0 : (ki == 1 ? 1.0 : h));
    c1[u] = kj == 0 ? 1.0 : (kj == 1 ? h : h2); c2[u] = kj == 0 ? 0.0 : (kj == 1 ? 1.0 : h);
  }
  // the lane's gradient entry (lanes < NV)
  const int lv = lane < NV ? lane : 0;
  const int kq = lv < NQ ? 0 : (lv < NX ? 1 : (lv >= NX + NS ? 2 : 3));
  const int iq = kq == 3 ? 0 : (kq == 0 ? lv : (kq == 1 ? lv - NQ : lv - NX - NS));
  const double l1q = kq == 3 ? 0.0 : (kq == 0 ? 1.0 : (kq == 1 ? h : h2)), l2q = kq == 3 ? 0.0 : (kq == 0 ? 0.0 : (kq == 1 ? 1.0 : h));
  const int lr = lane < NX ? lane : 0;
  // gains: lane c <= NX solves for column c of K (c < NX) or for kff (c == NX); sq follows sQ in the work area
  const int lc = lane <= NX ? lane : 0;
  // Every store of a phase is unconditional: a lane without an entry writes to a word of its own in the staging
  // area of the generic path (srec, unused here) instead of skipping the store -- a predicated store makes the
  // compiler cut the phase into exec-masked blocks with their own waits (15 of them per stage before).
  ldouble *const dummy = srec + lane;
  ldouble *qdst[EPL];
#pragma unroll
  for (int u = 0; u < EPL; u++) qdst[u] = (lane + LPI * u < NV * NV) ? sQ + lane + LPI * u : dummy;
  ldouble *const sqdst = lane < NV ? sq + lane : dummy;
  // cost-to-go entries of this lane (see the generic path): P(i, j) for e < NX*NX, then p(i)
  constexpr int PPL2 = (NX * NX + NX + LPI - 1) / LPI;
  int pa0[PPL2], pc0[PPL2], pqa[PPL2], pqc[PPL2], pka[PPL2], pkc[PPL2], pks[PPL2], pslot[PPL2];
  ldouble *pdst1[PPL2];
  bool pisP[PPL2], pok[PPL2];
#pragma unroll
  for (int u = 0; u < PPL2; u++) {
    const int e = lane + LPI * u;
    pok[u] = e < NX * NX + NX;
    const int ec = pok[u] ? e : 0;
    const bool isP = ec < NX * NX;
    pisP[u] = isP;
    const int i = isP ? ec / NX : ec - NX * NX, j = isP ? ec - i * NX : 0;
    // offsets relative to sQ (sq = sQ + NV*NV) and to the slot (K at 0, kff at OFF_KFF)
    pa0[u] = isP ? i * NV + j : NV * NV + i;
    pc0[u] = isP ? j * NV + i : NV * NV + i;
    pqa[u] = i * NV + NX;                          // sQ[i][NX + l]
    pqc[u] = isP ? j * NV + NX : i * NV + NX;      // cq[l]
    pka[u] = isP ? j : OFF_KFF;                    // K[l][j] = slot[l*NX + j]  |  kff[l] = slot[OFF_KFF + l]
    pkc[u] = isP ? i : OFF_KFF;
    pks[u] = isP ? NX : 1;                         // stride over l
    // where the entry goes: work area (sP / sp) and the stage's image (upper triangle of P packed, p); -1: nowhere
    pdst1[u] = !pok[u] ? dummy : (isP ? sP + ec : sp + (ec - NX * NX));
    pslot[u] = !pok[u] ? -1 : (isP ? (i <= j ? OFF_PT + ric_tri<NX>(i, j) : -1) : OFF_P + (ec - NX * NX));
  }
  for (int k = N - 1; k >= 0; k--) {
    ldouble *const slot = slots + (size_t)k * GS;   // record of stage k; becomes its image [K | kff | Pt | p | rc]
    // ---- phase A: stage Hessian and gradient, with [A|B]^T P [A|B] and [A|B]^T (P rc + p) in closed form ----
    double r0[EPL], r1[EPL], a11[EPL], a12[EPL], a21[EPL], a22[EPL];
#pragma unroll
    for (int u = 0; u < EPL; u++) {
      r0[u] = slot[qp[u]]; r1[u] = slot[cp[u]];
      a11[u] = sP[o11[u]]; a12[u] = sP[o11[u] + NQ]; a21[u] = sP[o11[u] + NQ * NX]; a22[u] = sP[o11[u] + NQ * NX + NQ];
    }
    double rcl[NX], pr1[NX], pr2[NX];
#pragma unroll
    for (int l = 0; l < NX; l++) { rcl[l] = slot[C::R_RC + l]; pr1[l] = sP[iq * NX + l]; pr2[l] = sP[(NQ + iq) * NX + l]; }
    double pc1 = sp[iq], pc2 = sp[NQ + iq];
    const double q0v = slot[C::R_Q0 + lv], q1v = slot[C::R_Q1 + lv], rcme = slot[C::R_RC + lr];
    __builtin_amdgcn_sched_barrier(0);   // (every read of the phase is issued before the first use: one counted wait instead of a wait per use)
#pragma unroll
    for (int u = 0; u < EPL; u++) {
      double v = r0[u] - cwt * r1[u];
      v += l1[u] * (c1[u] * a11[u] + c2[u] * a12[u]) + l2[u] * (c1[u] * a21[u] + c2[u] * a22[u]);
      *qdst[u] = v;
    }
#pragma unroll
    for (int l = 0; l < NX; l++) { pc1 += pr1[l] * rcl[l]; pc2 += pr2[l] * rcl[l]; }
    {
      double v = q0v - mu * q1v;
      v += l1q * pc1 + l2q * pc2;
      *sqdst = v;
    }
    *(lane < NX ? slot + OFF_RC + lane : dummy) = rcme;   // (behind the record: [OFF_RC, OFF_RC + NX) is step space, dead now)
    WSYNC();
    // ---- phase B: Cholesky of Qww (every lane, registers) and the gains (one column per lane) -------------
    double qw[NW][NW], colv[NW];
#pragma unroll
    for (int j = 0; j < NW; j++)
#pragma unroll
      for (int i = j; i < NW; i++) qw[i][j] = sQ[(NX + i) * NV + NX + j];
#pragma unroll
    for (int i = 0; i < NW; i++) colv[i] = sQ[lc < NX ? (NX + i) * NV + lc : NV * NV + NX + i];
    __builtin_amdgcn_sched_barrier(0);   // (every read of the phase is issued before the first use: one counted wait instead of a wait per use)
    double L[NW][NW], invd[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) {
      double dg = qw[j][j];
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
        double sacc = qw[i][j];
#pragma unroll
        for (int l = 0; l < j; l++) sacc -= L[i][l] * L[j][l];
        L[i][j] = sacc * inv;
      }
    }
    {
      double col[NW];
#pragma unroll
      for (int i = 0; i < NW; i++) col[i] = -colv[i];
      chol_solve<NW>(L, invd, col);
      {
        ldouble *const kdst = lane <= NX ? slot + (lane < NX ? lane : OFF_KFF) : dummy;
        const int kstr = lane < NX ? NX : (lane == NX ? 1 : 0);
#pragma unroll
        for (int i = 0; i < NW; i++) kdst[i * kstr] = col[i];
      }
    }
    WSYNC();
    // ---- phase C: cost-to-go P = sym(Qxx + Qxw K), p = qx + Qxw kff ---------------------------------------
    double pa[PPL2], pcc[PPL2], qa[PPL2][NW], qc[PPL2][NW], ka[PPL2][NW], kc[PPL2][NW];
#pragma unroll
    for (int u = 0; u < PPL2; u++) {
      pa[u] = sQ[pa0[u]]; pcc[u] = sQ[pc0[u]];
#pragma unroll
      for (int l = 0; l < NW; l++) {
        qa[u][l] = sQ[pqa[u] + l]; qc[u][l] = sQ[pqc[u] + l];
        ka[u][l] = slot[pka[u] + l * pks[u]]; kc[u][l] = slot[pkc[u] + l * pks[u]];
      }
    }
    __builtin_amdgcn_sched_barrier(0);   // (every read of the phase is issued before the first use: one counted wait instead of a wait per use)
#pragma unroll
    for (int u = 0; u < PPL2; u++) {
      double a = pa[u], c = pcc[u];
#pragma unroll
      for (int l = 0; l < NW; l++) {
        a += qa[u][l] * ka[u][l];
        c += qc[u][l] * kc[u][l];
      }
      const double pn = 0.5 * (a + c);
      *pdst1[u] = pn;                                      // work area: sP / sp, read by the next stage's phase A
      *(pslot[u] >= 0 ? slot + pslot[u] : dummy) = pn;     // image of the stage: packed triangle / p
    }
    WSYNC();   // (sP / sp of this stage are read by the next stage's phase A)
  }
  rst.start();   // (the phases of the rollout are stamped from here)
  return chol_ok;
}

// ---- fused kernel, diff-drive: backward pass with the structure of [A | B] used ------------------------------
// [A | B] of the unicycle is the identity outside the reduced block (x, y, theta, v, omega) = x[{0,1,2,6,7}] and its
// two input columns: T = P [A|B] has 7 computed columns (the identity columns are columns of P, the slack column
// is zero) and Q += [A|B]^T T has 7 computed rows, each a 5-term sum -- a third of the dense products, with the
// terms in the dense order (zeros and ones drop out exactly), so the values are those of the generic path.  The
// record entries a lane needs come straight from the record into its registers one stage ahead (no staging copy of
// the record in LDS), every producer stores its part of the gain image to the gain record itself (no read-back),
// and a stage has four ordering points instead of five.
template <class C, int LPI, class RP>
__device__ __forceinline__ bool ric_dd_backward(const RicCtx<C, LPI> &ctx, const RP *const rb, gdouble *const kpb, const int kps) {
  constexpr int NX = C::NX, NS = C::NS, NV = C::NV, NW = C::NW;
  constexpr int NP2 = RicCtx<C, LPI>::NP2, KPW = RicCtx<C, LPI>::KPW, EPL = RicCtx<C, LPI>::EPL;
  constexpr size_t sstr = C::RS;   // stage stride of the records
  const int N = ctx.N, lane = ctx.lane;
  const double mu = ctx.mu, cwt = ctx.cwt;
  ldouble *const img = ctx.img, *const sK = ctx.sK, *const skf = ctx.skf, *const sPt = ctx.sPt, *const sp = ctx.sp, *const src = ctx.src,
               *const sP = ctx.sP, *const sAB = ctx.sAB, *const sQ = ctx.sQ, *const sq = ctx.sq, *const sT = ctx.sT, *const sPc = ctx.sPc,
               *const srec = ctx.srec;
  const int (&qp)[EPL] = ctx.qp, (&cp)[EPL] = ctx.cp;
  bool chol_ok = true;
  constexpr int NR = 5, NT = NR + 2;            // reduced states; computed columns of T (reduced + inputs)
  constexpr int OFF_KFF = NW * NX, OFF_PT = NW * NX + NW, OFF_P = OFF_PT + NP2, OFF_RC = OFF_P + NX;
  ldouble *const sA5 = sAB, *const sB5 = sAB + 25, *const sZ = sAB + 35;   // sZ: one zero word
  ldouble *const sT7 = sT;                                                   // T[l][jc], 8 x 7
  auto Rl = [](int r) __attribute__((always_inline)) { return r < 3 ? r : r + 3; };        // reduced index -> state
  auto rid = [](int j) __attribute__((always_inline)) { return j < 3 ? j : (j >= 6 && j < 8 ? j - 3 : -1); };
  // phase A: entries of T this lane forms
  constexpr int TA = (NX * NT + LPI - 1) / LPI;
  int tpo[TA], tco[TA], tcs[TA], tst[TA];
  bool tok[TA];
#pragma unroll
  for (int u = 0; u < TA; u++) {
    const int t = lane + LPI * u;
    tok[u] = t < NX * NT;
    const int tc = tok[u] ? t : 0;
    const int i = tc / NT, jc = tc - i * NT;
    tpo[u] = i * NX;                                   // row i of P
    tco[u] = jc < NR ? jc : 25 + (jc - NR);            // M[rl][jc]: A5[rl][jc] | B5[rl][jc - 5]   (offset in sAB)
    tcs[u] = jc < NR ? NR : 2;
    tst[u] = tc;
  }
  // phase B: the lane's entries of the stage Hessian and its gradient entry
  int bto[EPL], bts[EPL], bco[EPL], bcs[EPL], bio[EPL];
  bool bok[EPL], bI[EPL];
  auto colsrc = [&](int j, int &to, int &ts) __attribute__((always_inline)) {
    // T[l][j] for l = 0..7: computed column | column of P | zero
    if (j < NX) {
      if (rid(j) >= 0) { to = (int)(sT7 - img) + rid(j); ts = NT; }
      else { to = (int)(sP - img) + j; ts = NX; }
    } else if (j >= NX + NS) { to = (int)(sT7 - img) + NR + (j - NX - NS); ts = NT; }
    else { to = (int)(sZ - img); ts = 0; }
  };
  auto rowsrc = [&](int i, int &co, int &cs, bool &isI) __attribute__((always_inline)) {
    // [A|B][l][i] for l in the reduced rows: column of A5 | column of B5 | nothing
    isI = false;
    if (i < NX) {
      if (rid(i) >= 0) { co = (int)(sA5 - img) + rid(i); cs = NR; }
      else { co = (int)(sZ - img); cs = 0; isI = true; }
    } else if (i >= NX + NS) { co = (int)(sB5 - img) + (i - NX - NS); cs = 2; }
    else { co = (int)(sZ - img); cs = 0; }
  };
#pragma unroll
  for (int u = 0; u < EPL; u++) {
    const int e = lane + LPI * u;
    bok[u] = e < NV * NV;
    const int ec = bok[u] ? e : 0;
    const int i = ec / NV, j = ec - i * NV;
    colsrc(j, bto[u], bts[u]);
    rowsrc(i, bco[u], bcs[u], bI[u]);
    bio[u] = bto[u] + (i < NX ? i : 0) * bts[u];      // T[i][j] (identity rows)
  }
  const int lq = lane < NV ? lane : 0;
  int qco, qcs;
  bool qI;
  rowsrc(lq, qco, qcs, qI);
  const int lr = lane < NX ? lane : 0;
  // record entries of the stage about to be processed, one stage ahead
  double rq[EPL], rqk[EPL], q0n = 0, q1n = 0, rcn = 0, abn[2] = {0, 0};
  auto fetch_dd = [&](int k) __attribute__((always_inline)) {
    const RP *const r = rb + (size_t)k * sstr;
#pragma unroll
    for (int u = 0; u < EPL; u++) { rq[u] = r[qp[u]]; rqk[u] = r[cp[u]]; }
    q0n = r[C::R_Q0 + lq]; q1n = r[C::R_Q1 + lq]; rcn = r[C::R_RC + lr];
#pragma unroll
    for (int u = 0; u < 2; u++) abn[u] = r[C::R_A5 + (lane + LPI * u < 35 ? lane + LPI * u : 0)];
  };
  // cost-to-go entries of this lane (as in the generic path): offsets of what an entry is made of, relative to the
  // work area (sQ, sq, sK, skf all live in it), and where it goes
  constexpr int PPL2 = (NX * NX + NX + LPI - 1) / LPI;
  // (the gain record always has a spare word behind the image: kps = (KPW + 8) / 8 * 8)
  // Every store of a phase is unconditional (a lane without an entry writes to a word of its own in the unused
  // staging area, or to the spare word behind the stage's gain record) and every read of a phase is issued before
  // its first use: a stage is straight-line code with one counted wait per phase instead of two dozen exec-masked
  // blocks that each wait for their own reads (as for the chain's path above).
  ldouble *const dummy = srec + lane;
  int da0[PPL2], dc0[PPL2], dqa[PPL2], dqc[PPL2], dka[PPL2], dkc[PPL2], dks[PPL2], dkp[PPL2];
  ldouble *dd1[PPL2], *dd2[PPL2];
#pragma unroll
  for (int u = 0; u < PPL2; u++) {
    const int e = lane + LPI * u;
    const bool okp = e < NX * NX + NX;
    const int ec = okp ? e : 0;
    const bool isP = ec < NX * NX;
    const int i = isP ? ec / NX : ec - NX * NX, j = isP ? ec - i * NX : 0;
    da0[u] = isP ? (int)(sQ - img) + i * NV + j : (int)(sq - img) + i;
    dc0[u] = isP ? (int)(sQ - img) + j * NV + i : (int)(sq - img) + i;
    dqa[u] = (int)(sQ - img) + i * NV + NX;
    dqc[u] = (int)(sQ - img) + (isP ? j : i) * NV + NX;
    dka[u] = isP ? (int)(sK - img) + j : (int)(skf - img);
    dkc[u] = isP ? (int)(sK - img) + i : (int)(skf - img);
    dks[u] = isP ? NX : 1;
    dd1[u] = !okp ? dummy : (isP ? sP + ec : sp + (ec - NX * NX));
    dd2[u] = (okp && isP && i <= j) ? sPt + ric_tri<NX>(i, j) : dummy;
    dkp[u] = !okp ? KPW : (isP ? (i <= j ? OFF_PT + ric_tri<NX>(i, j) : KPW) : OFF_P + (ec - NX * NX));
  }
  ldouble *tdst[TA];
#pragma unroll
  for (int u = 0; u < TA; u++) tdst[u] = tok[u] ? sT7 + tst[u] : dummy;
  ldouble *qdst[EPL];
#pragma unroll
  for (int u = 0; u < EPL; u++) qdst[u] = bok[u] ? sQ + lane + LPI * u : dummy;
  ldouble *const pcdst = lane < NX ? sPc + lane : dummy, *const sqdst = lane < NV ? sq + lane : dummy;
  ldouble *const srcdst = lane < NX ? src + lane : dummy;
  ldouble *abdst[2];
#pragma unroll
  for (int u = 0; u < 2; u++) abdst[u] = lane + LPI * u < 35 ? sAB + lane + LPI * u : dummy;
  const int lc = lane <= NX ? lane : 0;                           // gain column of this lane (NX: kff)
  ldouble *const kdst = lane <= NX ? img + (lane < NX ? lane : OFF_KFF) : dummy;
  const int kgo = lane <= NX ? (lane < NX ? lane : OFF_KFF) : KPW, kstr = lane < NX ? NX : (lane == NX ? 1 : 0);
  const int rco = lane < NX ? OFF_RC + lane : KPW;
  if (lane == 0) sZ[0] = 0.0;
  fetch_dd(N - 1);
  for (int k = N - 1; k >= 0; k--) {
    gdouble *const kpk = kpb + (size_t)k * kps;
    // this stage's record entries are in registers; the next one's leave now
    // (with the second-order terms of the unicycle: record entry minus the curvature entry when this step uses them)
    double rqc[EPL];
#pragma unroll
    for (int u = 0; u < EPL; u++) rqc[u] = rq[u] - cwt * rqk[u];
    const double q0c = q0n, q1c = q1n, rcc = rcn;
    // ([A5 | B5] and rc of THIS stage are in LDS since the last phase of the previous stage)
    if (k > 0) fetch_dd(k - 1);
    const bool rec_cost = k < N - 1;
    WSYNC();   // P, p of stage k+1 and [A5 | B5], rc of this stage are in LDS
    if (rec_cost) {
      // ---- phase A: T = P [A|B] (computed columns), Pc = P rc + p ------------------------------------------
      double ta[TA][NR], tb[TA][NR], pr[NX], rcl[NX];
#pragma unroll
      for (int u = 0; u < TA; u++)
#pragma unroll
        for (int r = 0; r < NR; r++) { ta[u][r] = sP[tpo[u] + Rl(r)]; tb[u][r] = sAB[tco[u] + r * tcs[u]]; }
#pragma unroll
      for (int l = 0; l < NX; l++) { pr[l] = sP[lr * NX + l]; rcl[l] = src[l]; }
      double pcv = sp[lr];
      __builtin_amdgcn_sched_barrier(0);
      double tv[TA];
#pragma unroll
      for (int u = 0; u < TA; u++) {
        double sacc = 0.0;
#pragma unroll
        for (int r = 0; r < NR; r++) sacc += ta[u][r] * tb[u][r];
        tv[u] = sacc;
      }
#pragma unroll
      for (int l = 0; l < NX; l++) pcv += pr[l] * rcl[l];
#pragma unroll
      for (int u = 0; u < TA; u++) *tdst[u] = tv[u];
      *pcdst = pcv;
      WSYNC();
    }
    // ---- phase B: Q = record + [A|B]^T T, q = q0 - mu q1 + [A|B]^T Pc ----------------------------------------
    {
      double qv[EPL];
      double gq = q0c - mu * q1c;
      if (rec_cost) {
        double ba[EPL][NR], bb[EPL][NR], bi[EPL], ga[NR], gb[NR];
#pragma unroll
        for (int u = 0; u < EPL; u++) {
#pragma unroll
          for (int r = 0; r < NR; r++) { ba[u][r] = img[bco[u] + r * bcs[u]]; bb[u][r] = img[bto[u] + Rl(r) * bts[u]]; }
          bi[u] = img[bio[u]];
        }
#pragma unroll
        for (int r = 0; r < NR; r++) { ga[r] = img[qco + r * qcs]; gb[r] = sPc[Rl(r)]; }
        const double gi = sPc[lq < NX ? lq : 0];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < EPL; u++) {
          double v = rqc[u];
#pragma unroll
          for (int r = 0; r < NR; r++) v += ba[u][r] * bb[u][r];
          v += bI[u] ? bi[u] : 0.0;
          qv[u] = v;
        }
#pragma unroll
        for (int r = 0; r < NR; r++) gq += ga[r] * gb[r];
        gq += qI ? gi : 0.0;
      } else {
#pragma unroll
        for (int u = 0; u < EPL; u++) qv[u] = rqc[u];
      }
#pragma unroll
      for (int u = 0; u < EPL; u++) *qdst[u] = qv[u];
      *sqdst = gq;
      kpk[rco] = rcc;   // the stage's defect: part of its gain image
    }
    WSYNC();
    // ---- phase C: Cholesky of Qww (every lane, registers) and the gains (one column per lane) ----------------
    {
      double qw[NW][NW], colv[NW];
#pragma unroll
      for (int j = 0; j < NW; j++)
#pragma unroll
        for (int i = j; i < NW; i++) qw[i][j] = sQ[(NX + i) * NV + NX + j];
#pragma unroll
      for (int i = 0; i < NW; i++) colv[i] = lc < NX ? sQ[(NX + i) * NV + lc] : sq[NX + i];
      __builtin_amdgcn_sched_barrier(0);
      double L[NW][NW], invd[NW];
#pragma unroll
      for (int j = 0; j < NW; j++) {
        double dg = qw[j][j];
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
          double sacc = qw[i][j];
#pragma unroll
          for (int l = 0; l < j; l++) sacc -= L[i][l] * L[j][l];
          L[i][j] = sacc * inv;
        }
      }
      double col[NW];
#pragma unroll
      for (int i = 0; i < NW; i++) col[i] = -colv[i];
      chol_solve<NW>(L, invd, col);
#pragma unroll
      for (int i = 0; i < NW; i++) {
        kdst[i * kstr] = col[i];
        kpk[kgo + i * kstr] = col[i];
      }
    }
    WSYNC();
    // ---- phase D: cost-to-go P = sym(Qxx + Qxw K), p = qx + Qxw kff; [A5 | B5], rc of the next stage to LDS -----
    {
      double a0[PPL2], c0[PPL2], qa[PPL2][NW], qc[PPL2][NW], ka[PPL2][NW], kc[PPL2][NW];
#pragma unroll
      for (int u = 0; u < PPL2; u++) {
        a0[u] = img[da0[u]]; c0[u] = img[dc0[u]];
#pragma unroll
        for (int l = 0; l < NW; l++) {
          qa[u][l] = img[dqa[u] + l]; qc[u][l] = img[dqc[u] + l];
          ka[u][l] = img[dka[u] + l * dks[u]]; kc[u][l] = img[dkc[u] + l * dks[u]];
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < PPL2; u++) {
        double a = a0[u], c = c0[u];
#pragma unroll
        for (int l = 0; l < NW; l++) {
          a += qa[u][l] * ka[u][l];
          c += qc[u][l] * kc[u][l];
        }
        const double pn = 0.5 * (a + c);
        *dd1[u] = pn;
        *dd2[u] = pn;
        kpk[dkp[u]] = pn;
      }
      // (what fetch_dd(k - 1) brought: nobody reads sAB / src again before the ordering point at the loop top;
      //  single-stage horizon: the forward pass reads the defect of stage 0 from the image)
#pragma unroll
      for (int u = 0; u < 2; u++) *(k > 0 ? abdst[u] : dummy) = abn[u];
      *srcdst = k > 0 ? rcn : rcc;
    }
  }
  return chol_ok;
}

// ---- the arms (pass kernels, one wavefront per instance, n = 5 .. 7 without slack): Schur-complement form ---------
// Round 4.  Stamps of the generic path on 1024 arms: stage Hessian 1.46 k, Cholesky + gains 1.44 k, cost-to-go 1.74 k
// cycles per backward stage, rollout 2.4 k per forward stage -- 134 LDS reads per lane and stage, five ordering
// points.  This path:
//   A  lane (i, j) of an n x n grid (8-lane groups) reads the four blocks S, T, T', V of the cost-to-go at (i, j) ONCE
//      and forms the seven block entries of [A|B]^T P [A|B] that are needed -- qq, qv, vq, vv in place over P, uq, uv,
//      uu for the control block -- instead of every dense entry fetching its four; its record entries come straight
//      from the stage record in global memory, requested one stage ahead (the record never passes through LDS);
//      g = P rc + p is summed over the 8 lanes of a group by DPP moves, and lanes j = 0, 1, 2 of group i finish
//      the gradient entries q_i, v_i, u_i: no separate gradient phase;
//   B  Cholesky of Quu in every lane (as before), then only the FORWARD substitution Y = L^-1 [Qux | qu] is on the
//      way to the next stage; the backward substitution that yields the gains K | kff goes to the image behind it;
//   C  P = Qxx - Y^T Y, p = qx - Y^T y on the matrix cores: two v_mfma_f64_16x16x4_f64 with the SAME register as
//      both operands (A = -Y^T, B = Y), accumulated onto [Qxx | qx]; the products of (i, j) and (j, i) are the same
//      numbers in the same order, and Qxx is formed symmetrically: the result is symmetric without the 0.5 (a + a^T).
// Three ordering points per backward stage, ~55 LDS reads per lane; the image of a stage is written where the
// rollout reads it.  The rollout forms dw, nu+ and dx+ from dx alone (one ordering point per stage: the lane of an
// entry of dx+ computes the entry of dw it needs itself), as the fused chain path does.
template <class C, class RP, class SP>
__device__ __forceinline__ bool ric_arm_block(const RicCtx<C, 64> &ctx, const RP *const rb, gdouble *const kpb, const int kps,
                                              const StepOut<SP> so, ldouble *const limg, const int lcap_rt) {
  // SP: where the step goes (the fused arm kernel keeps it in LDS while its records are in global memory);
  // lcap_rt >= 0: number of gain-image slots behind limg (the fused arm kernel; otherwise RicLds::IMG_SLOTS)
  constexpr int LPI = 64;
  constexpr int NQ = C::NQ, NX = C::NX, NW = C::NW;
  constexpr int NP2 = RicCtx<C, LPI>::NP2, KPW = RicCtx<C, LPI>::KPW, KPL = RicCtx<C, LPI>::KPL;
  constexpr int LCAP = RicLds<C, LPI>::IMG_SLOTS;   // stages 1 .. LCAP keep their image in LDS (limg)
  constexpr size_t sstr = C::RS;   // stage stride of the records
  const int N = ctx.N, lane = ctx.lane;
  const double h = ctx.h, h2 = ctx.h2, mu = ctx.mu, cwt = ctx.cwt;
  ldouble *const img = ctx.img;
  bool chol_ok = true;
  constexpr int n = NQ, PS = RicLds<C, LPI>::APS, QS = 16;
  constexpr int OFF_KFF = NW * NX, OFF_PT = OFF_KFF + NW, OFF_P = OFF_PT + NP2, OFF_RC = OFF_P + NX;
  static_assert(NW == n && NX == 2 * n && NX + 1 <= 16 && PS >= 16, "arm path: holonomic chain without slack, one MFMA tile");
  ldouble *const aP = img + KPW, *const aQux = aP + PS * NX, *const aQuu = aQux + QS * NW, *const aY = aQuu + 8 * NW,
               *const ap = aY + 128, *const adx = ap + 16, *const adum = adx + 32;
  ldouble *const dummy = adum + lane;
  const int LCAPr = lcap_rt >= 0 ? lcap_rt : LCAP;   // stages 1 .. LCAPr keep their image in LDS
  for (int e = lane; e < PS * NX; e += LPI) aP[e] = 0.0;   // P = 0 behind the last stage (columns NX, NX + 1: gradient / unused)
  aY[lane] = 0.0; aY[64 + lane] = 0.0;                     // (row 7 and column 15 of the operand tile stay zero)
  if (lane < 16) ap[lane] = 0.0;
  // -- lane (gi, gj): block position (ii, jj) ----------------------------------------------------------------
  const int gi = lane >> 3, gj = lane & 7;
  const bool gval = gi < n, gon = gval && gj < n;
  const int ii = gval ? gi : 0, jj = gj < n ? gj : 0;
  const bool gdiag = gon && ii == jj;
  const int qlo = ii < jj ? ii : jj, qhi = ii < jj ? jj : ii;
  const int tq = qlo * n - qlo * (qlo - 1) / 2 + (qhi - qlo);
  const int jme = gj == 0 ? ii : (gj == 1 ? n + ii : (gj == 2 ? 2 * n + ii : 0));   // gradient entry of lanes gj <= 2
  const double gc1 = gj == 0 ? 1.0 : (gj == 1 ? h : h2), gc2 = gj == 0 ? 0.0 : (gj == 1 ? 1.0 : h);
  int ro[8];   // record entries of this lane
  ro[0] = C::R_Q + tq; ro[1] = C::R_C + tq; ro[2] = C::R_DG + ii; ro[3] = C::R_DG + n + ii;
  ro[4] = C::R_RC + jj; ro[5] = C::R_RC + n + jj; ro[6] = C::R_Q0 + jme; ro[7] = C::R_Q1 + jme;
  const int oS = ii * PS + jj, oT = oS + n, oU = (n + ii) * PS + jj, oV = oU + n;
  ldouble *const dS = gon ? aP + oS : dummy, *const dT = gon ? aP + oT : dummy, *const dU = gon ? aP + oU : dummy,
               *const dV = gon ? aP + oV : dummy;
  ldouble *const dUq = gon ? aQux + ii * QS + jj : dummy, *const dUv = gon ? aQux + ii * QS + n + jj : dummy,
               *const dUu = gon ? aQuu + ii * 8 + jj : dummy;
  ldouble *const dq = (gval && gj <= 2) ? (gj == 2 ? aQux + ii * QS + NX : aP + (gj == 1 ? n + ii : ii) * PS + NX) : dummy;
  const bool rcw = lane < n;   // lanes (0, jj) put the defect of the stage into the image
  // -- phase B: gain column of this lane (NX: the gradient column) -------------------------------------------
  const int bc = lane <= NX ? lane : 0;
  const bool bon = lane <= NX;
  ldouble *const dY = bon ? aY + bc : dummy;
  const int ystr = bon ? 16 : 0;
  const int koff = lane < NX ? lane : (lane == NX ? OFF_KFF : -1), kstr = lane < NX ? NX : (lane == NX ? 1 : 0);
  // -- phase C: tile position of this lane -------------------------------------------------------------------
  typedef double v4d __attribute__((ext_vector_type(4)));
  const int c16 = lane & 15, kq = lane >> 4;
  int co[4], po2[4];
  bool cin[4];
  ldouble *cd1[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = kq + 4 * r;
    const bool rin = row < NX;
    cin[r] = rin;
    co[r] = (rin ? row : 0) * PS + c16;
    cd1[r] = !rin ? dummy : (c16 < NX ? aP + row * PS + c16 : (c16 == NX ? ap + row : dummy));
    po2[r] = !rin ? -1 : (c16 < NX ? (row <= c16 ? OFF_PT + ric_tri<NX>(row, c16) : -1) : (c16 == NX ? OFF_P + row : -1));
  }
  // record entries of the stage about to be processed, requested one stage ahead
  double rn[8];
#pragma unroll
  for (int u = 0; u < 8; u++) rn[u] = rb[(size_t)(N - 1) * sstr + ro[u]];
  RicStamps rst;
  rst.start();
  for (int k = N - 1; k >= 0; k--) {
    // image of this stage: stages 1 .. LCAP where the rollout reads them, the others in the staging area (stage 0
    // stays there; later ones leave for the gain record at the top of the next stage)
    ldouble *const imk = (k >= 1 && k <= LCAPr) ? limg + (size_t)(k - 1) * KPW : img;
    if (k + 1 < N && k + 1 > LCAPr) {   // (uniform) the image of stage k + 1 is complete in the staging area
      gdouble *const kp1 = kpb + (size_t)(k + 1) * kps;
#pragma unroll
      for (int u = 0; u < KPL; u++) {
        const int e = lane + LPI * u;
        kp1[e < KPW ? e : KPW] = img[e < KPW ? e : 0];   // (KPW: the record's spare word)
      }
    }
    double rc_[8];
#pragma unroll
    for (int u = 0; u < 8; u++) rc_[u] = rn[u];
    {
      const int kn = k > 0 ? k - 1 : 0;
#pragma unroll
      for (int u = 0; u < 8; u++) rn[u] = rb[(size_t)kn * sstr + ro[u]];   // travels while this stage is computed
    }
    rst(0);
    // ---- phase A -------------------------------------------------------------------------------------------
    {
      const double S = aP[oS], T = aP[oT], U = aP[oU], V = aP[oV], p1 = ap[ii], p2 = ap[n + ii];
      __builtin_amdgcn_sched_barrier(0);
      const double rcj = gj < n ? rc_[4] : 0.0, rcnj = gj < n ? rc_[5] : 0.0;
      const double tv = h * S + T, tu = h2 * S + h * T, bv = h * U + V, bu = h2 * U + h * V;
      const double qq = S + (rc_[0] - cwt * rc_[1]);
      const double vq = h * S + U;
      const double vv = (h * (h * S + (T + U)) + V) + (gdiag ? rc_[2] : 0.0);
      const double uq = h2 * S + h * U, uv = h2 * tv + h * bv;
      const double uu = (h2 * tu + h * bu) + (gdiag ? rc_[3] : 0.0);
      *dS = qq; *dT = tv; *dU = vq; *dV = vv;
      *dUq = uq; *dUv = uv; *dUu = uu;
      // g = P rc + p: the group's partial products, summed over its 8 lanes
      const double g1 = p1 + dpp_sum8(S * rcj + T * rcnj), g2 = p2 + dpp_sum8(U * rcj + V * rcnj);
      *dq = (rc_[6] - mu * rc_[7]) + (gc1 * g1 + gc2 * g2);
      *(rcw ? imk + OFF_RC + lane : dummy) = rc_[4];
      *(rcw ? imk + OFF_RC + n + lane : dummy) = rc_[5];
    }
    WSYNC();
    rst(1);
    // ---- phase B: Cholesky of Quu (every lane), Y = L^-1 [Qux | qu] (one column per lane), gains -------------
    v4d acc;
    {
      double qw[NW][NW], colv[NW], ac[4];
#pragma unroll
      for (int j = 0; j < NW; j++)
#pragma unroll
        for (int i = j; i < NW; i++) qw[i][j] = aQuu[i * 8 + j];
#pragma unroll
      for (int i = 0; i < NW; i++) colv[i] = aQux[i * QS + bc];
#pragma unroll
      for (int r = 0; r < 4; r++) ac[r] = aP[co[r]];   // (accumulator of phase C: arrives during the factorisation)
      __builtin_amdgcn_sched_barrier(0);
      double L[NW][NW], invd[NW];
#pragma unroll
      for (int j = 0; j < NW; j++) {
        double dg = qw[j][j];
#pragma unroll
        for (int l = 0; l < j; l++) dg -= L[j][l] * L[j][l];
        if (!(dg > 0.0)) chol_ok = false;
        // 1/sqrt(dg): hardware estimate + two Newton steps (full double precision), then sqrt = dg * rsqrt
        double inv = __builtin_amdgcn_rsq(dg);
        inv = inv * (1.5 - 0.5 * dg * inv * inv);
        inv = inv * (1.5 - 0.5 * dg * inv * inv);
        L[j][j] = dg * inv;
        invd[j] = inv;
#pragma unroll
        for (int i = j + 1; i < NW; i++) {
          double s = qw[i][j];
#pragma unroll
          for (int l = 0; l < j; l++) s -= L[i][l] * L[j][l];
          L[i][j] = s * inv;
        }
      }
      double y[NW];
#pragma unroll
      for (int i = 0; i < NW; i++) {
        double s = colv[i];
#pragma unroll
        for (int l = 0; l < i; l++) s -= L[i][l] * y[l];
        y[i] = s * invd[i];
        dY[i * ystr] = y[i];
      }
#pragma unroll
      for (int r = 0; r < 4; r++) acc[r] = cin[r] ? ac[r] : 0.0;
      WSYNC();
      rst(3);
      // ---- phase C: [P | p] = [Qxx | qx] - Y^T [Y | y] --------------------------------------------------------
      const double ya = aY[kq * 16 + c16], yb = aY[(4 + kq) * 16 + c16];
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-ya, ya, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-yb, yb, acc, 0, 0, 0);
      // (behind the matrix instructions: the gains K = -L^-T Y of this lane's column, for the rollout only)
      double x[NW];
#pragma unroll
      for (int i = NW - 1; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int l = i + 1; l < NW; l++) s -= L[l][i] * x[l];
        x[i] = s * invd[i];
      }
      ldouble *const kd = koff >= 0 ? imk + koff : dummy;
#pragma unroll
      for (int i = 0; i < NW; i++) kd[i * kstr] = -x[i];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        *cd1[r] = acc[r];
        *(po2[r] >= 0 ? imk + po2[r] : dummy) = acc[r];
      }
    }
    WSYNC();   // (P, p of this stage are read by the next stage's phase A)
    rst(4);
  }
  if (!chol_ok) return false;
  // ---- rollout: dw = kff + K dx, nu+ = p + P dx, dx+ = rc + [A|B][dx; dw], one ordering point per stage --------
  const bool fA = lane < NW, fB = lane >= NW && lane < NW + NX, fC = lane >= NW + NX && lane < NW + 2 * NX;
  const int fi = fA ? lane : (fB ? lane - NW : (fC ? lane - NW - NX : 0));   // entry of dw / nu+ / dx+
  const int fw = fC ? (fi < n ? fi : fi - n) : fi;                             // the entry of dw a dx+ lane needs
  const int foff = fB ? OFF_P + fi : OFF_KFF + fw;
  int frow[NX];
#pragma unroll
  for (int j = 0; j < NX; j++) frow[j] = fB ? OFF_PT + ric_tri<NX>(fi, j) : fw * NX + j;
  const int fx1 = fi < n ? n + fi : fi;
  const double fca = fi < n ? h : 0.0, fcb = fi < n ? h2 : h;
  const size_t dzslot = fA ? (size_t)(NX + lane) : (size_t)fi;
  if (lane < 32) adx[lane] = 0.0;
  constexpr int FD = 4;
  double fvq[FD][KPL];
  auto fetch_fwd = [&](int k, double (&fv)[KPL]) __attribute__((always_inline)) {
    const int kk = k < N ? k : N - 1;
#pragma unroll
    for (int u = 0; u < KPL; u++) {
      const int e = lane + LPI * u;
      fv[u] = kpb[(size_t)kk * kps + (e < KPW ? e : 0)];
    }
  };
#pragma unroll
  for (int d = 0; d < FD; d++) fetch_fwd(LCAPr + 1 + d, fvq[d]);
  auto fwd_stage = [&](const int k, double (&fv)[KPL], const bool from_mem) __attribute__((always_inline)) {
    const ldouble *const im = (!from_mem && k > 0) ? limg + (size_t)(k - 1) * KPW : img;
    if (from_mem) {
#pragma unroll
      for (int u = 0; u < KPL; u++) *(lane + LPI * u < KPW ? img + lane + LPI * u : dummy) = fv[u];
      fetch_fwd(k + FD, fv);
    }
    const ldouble *const dxc = adx + 16 * (k & 1);
    ldouble *const dxn = adx + 16 * ((k & 1) ^ 1);
    WSYNC();
    rst(5);
    double dxv[NX], rowv[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) { dxv[j] = dxc[j]; rowv[j] = im[frow[j]]; }
    double sacc = im[foff];
    const double rcv = im[OFF_RC + fi], d0 = dxc[fi], d1 = dxc[fx1];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NX; j++) sacc += rowv[j] * dxv[j];
    // (unconditional stores, idle lanes to the spare word of the stage's gain record)
    SP *sink;
    if constexpr (std::is_same<SP, ldouble>::value) sink = dummy;
    else sink = (SP *)(kpb + (size_t)k * kps + KPW);
    *((fA || fC) ? so.dz + dzslot * so.SS + (size_t)k * so.KS : sink) = fA ? sacc : d0;
    *((fB && k >= 1) ? so.nunew + (size_t)fi * so.SS + (size_t)k * so.KS : sink) = sacc;
    double sx = rcv;
    sx += d0;
    sx += fca * d1;
    sx += fcb * sacc;
    *((fC && k < N - 1) ? dxn + fi : dummy) = sx;
    rst(6);
  };
  for (int k = 0; k < N && k <= LCAPr; k++) fwd_stage(k, fvq[0], false);
  for (int k0 = LCAPr + 1; k0 < N; k0 += FD) {
#pragma unroll
    for (int d = 0; d < FD; d++) {
      if (k0 + d < N) fwd_stage(k0 + d, fvq[d], true);   // (uniform branch)
    }
  }
  rst.flush(lane);
  return true;
}

template <class C, int LPI, class RP>
__device__ __forceinline__ bool ric_backward(const RicCtx<C, LPI> &ctx, const RP *const rb, gdouble *const kpb, const int kps,
                                             ldouble *const limg, RicStamps &rst) {
  constexpr int NQ = C::NQ, NX = C::NX, NS = C::NS, NV = C::NV, NW = C::NW;
  constexpr bool DD = RicCtx<C, LPI>::DD;
  constexpr int KPW = RicCtx<C, LPI>::KPW, KPL = RicCtx<C, LPI>::KPL, EPL = RicCtx<C, LPI>::EPL;
  constexpr int TPL = RicCtx<C, LPI>::TPL, RPL = RicCtx<C, LPI>::RPL;
  constexpr bool LIMG = RicLds<C, LPI>::LIMG;
  constexpr int LCAP = LIMG ? RicLds<C, LPI>::IMG_SLOTS : 0;   // stages 1 .. LCAP keep their image in LDS (limg)
  constexpr size_t sstr = C::RS;   // stage stride of the records
  // the arms' cost-to-go update on the matrix cores (v_mfma_f64_16x16x4_f64): one wavefront per instance, a state of
  // 9 .. 15 entries (one tile with the gradient column), at most 8 inputs (two k-steps)
  constexpr bool MFMA_P = !DD && LPI == 64 && NX > 8 && NX < 16 && NW <= 8;
  const int N = ctx.N, lane = ctx.lane;
  const double h = ctx.h, h2 = ctx.h2, mu = ctx.mu, cwt = ctx.cwt;
  ldouble *const img = ctx.img, *const sK = ctx.sK, *const skf = ctx.skf, *const sPt = ctx.sPt, *const sp = ctx.sp, *const src = ctx.src,
               *const sP = ctx.sP, *const sAB = ctx.sAB, *const sQ = ctx.sQ, *const sq = ctx.sq, *const sT = ctx.sT, *const sPc = ctx.sPc,
               *const srec = ctx.srec;
  const int (&qp)[EPL] = ctx.qp, (&cp)[EPL] = ctx.cp;
  bool chol_ok = true;
  // prefetched record of the stage about to be processed (lane e holds entry e)
  double recv[RPL];
  auto fetch_stage = [&](int k) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < RPL; u++) {
      const int e = lane + LPI * u;
      recv[u] = rb[(size_t)k * sstr + (e < C::RS ? e : 0)];
    }
  };
  // [A|B] of the stage whose record is in srec
  auto fill_AB_dd = [&]() __attribute__((always_inline)) {
    if constexpr (DD) {
#pragma unroll
      for (int u = 0; u < TPL; u++) {
        const int e = lane + LPI * u;
        const double v = srec[ctx.abp[u]] + ctx.abc[u];
        if (e < NX * NV) sAB[e] = v;
      }
    }
  };
  // ---- per-lane constants --------------------------------------------------------------------------------------
  // idle lanes store to a word of the unused T area (several lanes may share one: the value is never read)
  ldouble *const gdummy = sT + lane % RicLds<C, LPI>::TW;
  ldouble *gsrdst[RPL];
#pragma unroll
  for (int u = 0; u < RPL; u++) gsrdst[u] = lane + LPI * u < C::RS ? srec + lane + LPI * u : gdummy;
  int go11[EPL];
  double gl1[EPL], gl2[EPL], gc1[EPL], gc2[EPL];
  bool gon[EPL];
  ldouble *gqdst[EPL];
#pragma unroll
  for (int u = 0; u < EPL; u++) {
    const int e = lane + LPI * u;
    const bool ok = e < NV * NV;
    const int ec = ok ? e : 0;
    const int i = ec / NV, j = ec - i * NV;
    // row / column kind: 0 = q, 1 = v, 2 = u, 3 = slack (no contribution)
    const int ki = i < NQ ? 0 : (i < NX ? 1 : (i >= NX + NS ? 2 : 3));
    const int kj = j < NQ ? 0 : (j < NX ? 1 : (j >= NX + NS ? 2 : 3));
    gon[u] = ok && ki != 3 && kj != 3;
    const int ii = !gon[u] ? 0 : (ki == 0 ? i : (ki == 1 ? i - NQ : i - NX - NS));
    const int jj = !gon[u] ? 0 : (kj == 0 ? j : (kj == 1 ? j - NQ : j - NX - NS));
    go11[u] = ii * NX + jj;
    // left factor: row kind picks the combination of the two block rows -- q: (1, 0); v: (h, 1); u: (h2, h)
    gl1[u] = ki == 0 ? 1.0 : (ki == 1 ? h : h2); gl2[u] = ki == 0 ? 0.0 : (ki == 1 ? 1.0 : h);
    gc1[u] = kj == 0 ? 1.0 : (kj == 1 ? h : h2); gc2[u] = kj == 0 ? 0.0 : (kj == 1 ? 1.0 : h);
    gqdst[u] = ok ? sQ + e : gdummy;
  }
  const int glr = lane < NX ? lane : 0, glv = lane < NV ? lane : 0;
  ldouble *const gsrc = lane < NX ? src + lane : gdummy, *const gpcdst = lane < NX ? sPc + lane : gdummy;
  ldouble *const gsqdst = lane < NV ? sq + lane : gdummy;
  const int gkq = glv < NQ ? 0 : (glv < NX ? 1 : (glv >= NX + NS ? 2 : 3));
  const bool gqon = lane < NV && gkq != 3;
  const int giq = !gqon ? 0 : (gkq == 0 ? glv : (gkq == 1 ? glv - NQ : glv - NX - NS));
  const double gl1q = gkq == 0 ? 1.0 : (gkq == 1 ? h : h2), gl2q = gkq == 0 ? 0.0 : (gkq == 1 ? 1.0 : h);
  const int glc = lane <= NX ? lane : 0;   // gain column of this lane (NX: kff)
  ldouble *const gkdst = lane <= NX ? (lane < NX ? sK + lane : skf) : gdummy;
  const int gkstr = lane < NX ? NX : (lane == NX ? 1 : 0);
  fetch_stage(N - 1);
  rst.start();
  for (int k = N - 1; k >= 0; k--) {
    // -- the image of stage k+1 is complete: it leaves for the gain record (read now, stored after the
    //    barrier); the stage record goes to LDS, the request for the next one leaves ----------------
    double kpv[KPL];
#pragma unroll
    for (int u = 0; u < KPL; u++) {
      const int e = lane + LPI * u;
      kpv[u] = img[e < KPW ? e : 0];
    }
#pragma unroll
    for (int u = 0; u < RPL; u++) *gsrdst[u] = recv[u];
    if (k > 0) fetch_stage(k - 1);  // travels while this stage is computed
    WSYNC();
    rst(0);
    if (k < N - 1) {
      if (LIMG && k + 1 <= LCAP) {
        ldouble *const kl = limg + (size_t)k * KPW;   // (slot of stage k + 1)
#pragma unroll
        for (int u = 0; u < KPL; u++) *(lane + LPI * u < KPW ? kl + lane + LPI * u : gdummy) = kpv[u];
      } else {
        gdouble *const kp1 = kpb + (size_t)(k + 1) * kps;
#pragma unroll
        for (int u = 0; u < KPL; u++) kp1[lane + LPI * u < KPW ? lane + LPI * u : KPW] = kpv[u];   // (KPW: the record's spare word)
      }
    }
    if constexpr (!DD) {
      // Holonomic chain: A = [I hI; 0 I], B = [h2 I; h I].  The dense stage Hessian is formed in one step
      // from the record blocks and [A|B]^T P [A|B] in closed form (each entry from at most four entries of
      // P: blocks 11, 12, 21, 22 at (ii, jj)); rc of the stage goes into the image (stage N-1: finite, unused).
      // Straight-line phases: what an entry is made of and where it goes are loop-invariant per-lane constants
      // (go*), every read of a phase is issued before its first use, every store is unconditional (idle lanes write
      // to gdummy) -- as for the fused kernel's paths above; same arithmetic per entry.
      const bool rec_cost = k < N - 1;   // a cost-to-go of stage k+1 exists
      {
        double r0[EPL], r1[EPL], a11[EPL], a12[EPL], a21[EPL], a22[EPL], pr[NX], rcl[NX];
#pragma unroll
        for (int u = 0; u < EPL; u++) {
          r0[u] = srec[qp[u]]; r1[u] = srec[cp[u]];
          a11[u] = sP[go11[u]]; a12[u] = sP[go11[u] + NQ]; a21[u] = sP[go11[u] + NQ * NX]; a22[u] = sP[go11[u] + NQ * NX + NQ];
        }
#pragma unroll
        for (int l = 0; l < NX; l++) { pr[l] = sP[glr * NX + l]; rcl[l] = srec[C::R_RC + l]; }
        const double rcme = srec[C::R_RC + glr];
        double pcs = sp[glr];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < EPL; u++) {
          double v = r0[u] - cwt * r1[u];
          const double add = gl1[u] * (gc1[u] * a11[u] + gc2[u] * a12[u]) + gl2[u] * (gc1[u] * a21[u] + gc2[u] * a22[u]);
          v = (rec_cost && gon[u]) ? v + add : v;
          *gqdst[u] = v;
        }
#pragma unroll
        for (int l = 0; l < NX; l++) pcs += pr[l] * rcl[l];
        *gsrc = rcme;
        *gpcdst = pcs;     // (stage N-1: P = 0, p = 0 -- the product is not used)
      }
      WSYNC();
      rst(1);
      {
        const double q0v = srec[C::R_Q0 + glv], q1v = srec[C::R_Q1 + glv], pc1 = sPc[giq], pc2 = sPc[NQ + giq];
        __builtin_amdgcn_sched_barrier(0);
        double v = q0v - mu * q1v;
        v = (rec_cost && gqon) ? v + (gl1q * pc1 + gl2q * pc2) : v;
        *gsqdst = v;
      }
      WSYNC();
      rst(2);
    } else {
      // -- fill: dense stage Hessian, gradient, defect (rc of stage N-1: finite, unused), [A|B] -------
#pragma unroll
      for (int u = 0; u < EPL; u++) {
        const int e = lane + LPI * u;
        const double v = srec[qp[u]] - cwt * srec[cp[u]];
        if (e < NV * NV) sQ[e] = v;
      }
      if (lane < NV) sq[lane] = srec[C::R_Q0 + lane] - mu * srec[C::R_Q1 + lane];
      if (lane < NX) src[lane] = srec[C::R_RC + lane];
      if (k < N - 1) fill_AB_dd();
      WSYNC();
      if (k < N - 1) {
      // -- T = P [A|B], Pc = P rc + p ---------------------------------------------------------
#pragma unroll
      for (int u = 0; u < TPL; u++) {
        const int e = lane + LPI * u;
        if (e < NX * NV) {
          const int i = e / NV, j = e - i * NV;
          double s = 0.0;
#pragma unroll
          for (int l = 0; l < NX; l++) s += sP[i * NX + l] * sAB[l * NV + j];
          sT[e] = s;
        }
      }
      if (lane < NX) {
        double s = sp[lane];
#pragma unroll
        for (int l = 0; l < NX; l++) s += sP[lane * NX + l] * src[l];
        sPc[lane] = s;
      }
      WSYNC();
      // -- Q += [A|B]^T T, q += [A|B]^T Pc ---------------------------------------------------------
#pragma unroll
      for (int u = 0; u < EPL; u++) {
        const int e = lane + LPI * u;
        if (e < NV * NV) {
          const int i = e / NV, j = e - i * NV;
          double s = sQ[e];
#pragma unroll
          for (int l = 0; l < NX; l++) s += sAB[l * NV + i] * sT[l * NV + j];
          sQ[e] = s;
        }
      }
      if (lane < NV) {
        double s = sq[lane];
#pragma unroll
        for (int l = 0; l < NX; l++) s += sAB[l * NV + lane] * sPc[l];
        sq[lane] = s;
      }
      WSYNC();
      }
    }
    // -- Cholesky of Qww: every lane factors the small block in registers (its entries and the lane's right-hand
    //    side are requested first, all at once) -----------------------------------------------------------------
    double qw[NW][NW], colv[NW];
#pragma unroll
    for (int j = 0; j < NW; j++)
#pragma unroll
      for (int i = j; i < NW; i++) qw[i][j] = sQ[(NX + i) * NV + NX + j];
#pragma unroll
    for (int i = 0; i < NW; i++) colv[i] = glc < NX ? sQ[(NX + i) * NV + glc] : sq[NX + i];
    __builtin_amdgcn_sched_barrier(0);
    double L[NW][NW], invd[NW];
#pragma unroll
    for (int j = 0; j < NW; j++) {
      double dg = qw[j][j];
#pragma unroll
      for (int l = 0; l < j; l++) dg -= L[j][l] * L[j][l];
      if (!(dg > 0.0)) chol_ok = false;
      // 1/sqrt(dg): hardware estimate + two Newton steps (full double precision), then sqrt = dg * rsqrt
      double inv = __builtin_amdgcn_rsq(dg);
      inv = inv * (1.5 - 0.5 * dg * inv * inv);
      inv = inv * (1.5 - 0.5 * dg * inv * inv);
      L[j][j] = dg * inv;
      invd[j] = inv;
#pragma unroll
      for (int i = j + 1; i < NW; i++) {
        double s = qw[i][j];
#pragma unroll
        for (int l = 0; l < j; l++) s -= L[i][l] * L[j][l];
        L[i][j] = s * inv;
      }
    }
    // -- gains: lane c < NX solves for column c of K, lane NX for kff (the other lanes solve column 0 again and
    //    store to gdummy) ---------------------------------------------------------------------------------------
    {
      double col[NW];
#pragma unroll
      for (int i = 0; i < NW; i++) col[i] = -colv[i];
      chol_solve<NW>(L, invd, col);
#pragma unroll
      for (int i = 0; i < NW; i++) gkdst[i * gkstr] = col[i];
    }
    WSYNC();
    rst(3);
    // -- cost-to-go: P = sym(Qxx + Qxw K), p = qx + Qxw kff ---------------------------------------------
    if constexpr (MFMA_P) {
      // The arms, one wavefront per instance: the 14 x 7 x 15 product on the matrix cores.  M = Qxw [K | kff] is one
      // 16 x 16 tile of v_mfma_f64_16x16x4_f64 (two k-steps of four), accumulated onto C = [Qxx | qx]; its transpose
      // M^T = [K | kff]^T Qxw^T comes from the same two operand registers swapped, accumulated onto Qxx^T, so that
      // a lane holds M(i, j) and M(j, i) for its four entries: 14 LDS reads and 4 matrix instructions per lane
      // instead of 120 reads and 56 multiply-adds (the sums keep the order l = 0 .. NW-1 on top of the Qxx entry).
      // Operand maps (guide, "Fragment layout"): A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
      // C / D[row = (lane >> 4) + 4 r][col = lane & 15], r = 0 .. 3.
      typedef double v4d __attribute__((ext_vector_type(4)));
      const int c16 = lane & 15, kq = lane >> 4;
      const bool cin = c16 < NX;
      const int cc = cin ? c16 : 0;
      double a0 = sQ[cc * NV + NX + kq];                                   // Qxw(c16, kq)
      double a1 = sQ[cc * NV + NX + (4 + kq < NW ? 4 + kq : 0)];           // Qxw(c16, 4 + kq)
      double b0 = c16 == NX ? skf[kq] : sK[kq * NX + cc];                  // K(kq, c16) | kff(kq)
      double b1 = c16 == NX ? skf[4 + kq < NW ? 4 + kq : 0] : sK[(4 + kq < NW ? 4 + kq : 0) * NX + cc];
      a0 = cin ? a0 : 0.0;
      a1 = (cin && 4 + kq < NW) ? a1 : 0.0;
      b0 = c16 <= NX ? b0 : 0.0;
      b1 = (c16 <= NX && 4 + kq < NW) ? b1 : 0.0;
      v4d cacc, tacc;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = kq + 4 * r;
        const bool rin = row < NX;
        const int rr = rin ? row : 0;
        const double qe = sQ[rr * NV + cc], qt = sQ[cc * NV + rr], qv = sq[rr];
        cacc[r] = !rin ? 0.0 : (cin ? qe : (c16 == NX ? qv : 0.0));
        tacc[r] = (rin && cin) ? qt : 0.0;
      }
      cacc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, cacc, 0, 0, 0);
      tacc = __builtin_amdgcn_mfma_f64_16x16x4f64(b0, a0, tacc, 0, 0, 0);
      cacc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, cacc, 0, 0, 0);
      tacc = __builtin_amdgcn_mfma_f64_16x16x4f64(b1, a1, tacc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = kq + 4 * r;
        if (row < NX) {
          if (cin) {
            const double pn = 0.5 * (cacc[r] + tacc[r]);
            sP[row * NX + c16] = pn;
            if (row <= c16) sPt[ric_tri<NX>(row, c16)] = pn;
          } else if (c16 == NX) {
            sp[row] = cacc[r];
          }
        }
      }
    } else {
    // entries e < NX*NX are P(i, j); the next NX entries are p(i), written as the same expression with the
    // "column" kff and no transposed partner (a == c, 0.5 (a + a) = a exactly): one instruction stream
    constexpr int PPL2 = (NX * NX + NX + LPI - 1) / LPI;
    double pn[PPL2];
#pragma unroll
    for (int u = 0; u < PPL2; u++) {
      const int e = lane + LPI * u;
      pn[u] = 0.0;
      if (e < NX * NX + NX) {
        const bool isP = e < NX * NX;
        const int i = isP ? e / NX : e - NX * NX, j = isP ? e - i * NX : 0;
        const ldouble *const a0 = isP ? sQ + i * NV + j : sq + i;
        const ldouble *const c0 = isP ? sQ + j * NV + i : sq + i;
        const ldouble *const cq = isP ? sQ + j * NV + NX : sQ + i * NV + NX;
        double a = *a0, c = *c0;
#pragma unroll
        for (int l = 0; l < NW; l++) {
          a += sQ[i * NV + NX + l] * (isP ? sK[l * NX + j] : skf[l]);
          c += cq[l] * (isP ? sK[l * NX + i] : skf[l]);
        }
        pn[u] = 0.5 * (a + c);
      }
    }
    // (no ordering point needed: what is written now -- sP, sPt, sp -- is not read in this phase, and the
    //  LDS instructions of a wavefront execute in program order)
#pragma unroll
    for (int u = 0; u < PPL2; u++) {
      const int e = lane + LPI * u;
      if (e < NX * NX) {
        sP[e] = pn[u];
        const int i = e / NX, j = e - i * NX;
        if (i <= j) sPt[ric_tri<NX>(i, j)] = pn[u];
      } else if (e < NX * NX + NX) {
        sp[e - NX * NX] = pn[u];
      }
    }
    }
    // (the fill of the next stage touches sQ / sq / src only; its barrier orders the sP writes)
    rst(4);
  }
  return chol_ok;
}

// ---- fused kernel, diff-drive: forward rollout with ONE ordering point per stage ---------------------------------
// As in the chain's path, the lane that forms an entry of dx+ computes the two input steps it needs itself (same
// expression, same value as the lane that stores them); dx ping-pongs between two buffers; the image and [A5 | B5]
// of the next stage travel from the gain record / the stage record while this stage is computed; the products
// with [A | B] keep only its non-trivial entries, in the dense order.
template <class C, int LPI, class RP>
__device__ __forceinline__ void ric_dd_rollout(const RicCtx<C, LPI> &ctx, const RP *const rb, const gdouble *const kpb,
                                               const int kps, const StepOut<gdouble> so) {
  constexpr int NX = C::NX, NS = C::NS, NW = C::NW;
  constexpr int NP2 = RicCtx<C, LPI>::NP2, KPW = RicCtx<C, LPI>::KPW, KPL = RicCtx<C, LPI>::KPL;
  constexpr size_t sstr = C::RS;   // stage stride of the records
  const int N = ctx.N, lane = ctx.lane;
  ldouble *const img = ctx.img, *const sAB = ctx.sAB, *const sPc = ctx.sPc, *const sdx = ctx.sdx, *const srec = ctx.srec;
  constexpr int NR = 5;
  constexpr int OFF_KFF = NW * NX, OFF_PT = NW * NX + NW, OFF_P = OFF_PT + NP2, OFF_RC = OFF_P + NX;
  ldouble *const dx0 = sdx, *const dx1 = sPc;
  auto Rl = [](int r) __attribute__((always_inline)) { return r < 3 ? r : r + 3; };
  auto rid = [](int j) __attribute__((always_inline)) { return j < 3 ? j : (j >= 6 && j < 8 ? j - 3 : -1); };
  double fv[KPL], abf[2] = {0, 0};
  auto fetch_f = [&](int k) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < KPL; u++) {
      const int e = lane + LPI * u;
      fv[u] = kpb[(size_t)k * kps + (e < KPW ? e : 0)];
    }
#pragma unroll
    for (int u = 0; u < 2; u++) abf[u] = rb[(size_t)k * sstr + C::R_A5 + (lane + LPI * u < 35 ? lane + LPI * u : 0)];
  };
  WSYNC();
  if (lane < NX) dx0[lane] = 0.0;
  if (N > 1) fetch_f(1);
  // role of the lane in the "offset + row . dx" stream: an input / slack step (lanes < NW) or a costate
  const bool isw = lane < NW, isn = lane >= NW && lane < NW + NX;
  const int in = isn ? lane - NW : 0;
  int ro[NX];
#pragma unroll
  for (int j = 0; j < NX; j++) ro[j] = isw ? lane * NX + j : OFF_PT + ric_tri<NX>(in, j);
  const int oo = isw ? OFF_KFF + lane : OFF_P + in;
  // dx+ entry of the lane
  const int lx = lane < NX ? lane : 0;
  const bool xI = rid(lx) < 0;
  const int ao = xI ? 35 : rid(lx) * NR, as = xI ? 0 : 1;   // row of A5 (offsets in sAB; 35 = the zero word)
  const int bo = xI ? 35 : 25 + rid(lx) * 2, bs = xI ? 0 : 1;
  // (unconditional stores and batched reads as in the backward pass)
  ldouble *const fdummy = srec + lane;
  ldouble *fdst[KPL], *fab[2];
#pragma unroll
  for (int u = 0; u < KPL; u++) fdst[u] = lane + LPI * u < KPW ? img + lane + LPI * u : fdummy;
#pragma unroll
  for (int u = 0; u < 2; u++) fab[u] = lane + LPI * u < 35 ? sAB + lane + LPI * u : fdummy;
  // (the two global stores of the step stay predicated: there is no spare word in the step arrays)
  for (int k = 0; k < N; k++) {
    const ldouble *const dxc = (k & 1) ? dx1 : dx0;
    ldouble *const dxn = (k & 1) ? dx0 : dx1;
    // image and [A5 | B5] of this stage (what the previous iteration requested; stage 0's are in place)
#pragma unroll
    for (int u = 0; u < KPL; u++) *(k > 0 ? fdst[u] : fdummy) = fv[u];
#pragma unroll
    for (int u = 0; u < 2; u++) *(k > 0 ? fab[u] : fdummy) = abf[u];
    if (k + 1 < N) fetch_f(k + 1);
    WSYNC();
    double dx[NX], rw[NX], ku[2][NX], ar[NR], br[2];
#pragma unroll
    for (int j = 0; j < NX; j++) { dx[j] = dxc[j]; rw[j] = img[ro[j]]; }
    const double own0 = img[oo];
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int j = 0; j < NX; j++) ku[c][j] = img[(NS + c) * NX + j];
    const double kf0 = img[OFF_KFF + NS], kf1 = img[OFF_KFF + NS + 1];
#pragma unroll
    for (int r = 0; r < NR; r++) ar[r] = sAB[ao + r * as];
#pragma unroll
    for (int c = 0; c < 2; c++) br[c] = sAB[bo + c * bs];
    const double rcv = img[OFF_RC + lx];
    const double dxo = dxc[in], dxme = dxc[lx];
    __builtin_amdgcn_sched_barrier(0);
    // own entry of the step / costate
    double sown = own0;
#pragma unroll
    for (int j = 0; j < NX; j++) sown += rw[j] * dx[j];
    // the two input steps (every lane: the dx+ lanes need them)
    double du[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
      double sacc = c == 0 ? kf0 : kf1;
#pragma unroll
      for (int j = 0; j < NX; j++) sacc += ku[c][j] * dx[j];
      du[c] = sacc;
    }
    if (lane < NW + NX) so.dz[(size_t)(isw ? NX + lane : in) * so.SS + (size_t)k * so.KS] = isw ? sown : dxo;
    if (isn && k >= 1) so.nunew[(size_t)in * so.SS + (size_t)k * so.KS] = sown;
    {
      double sx = rcv;
#pragma unroll
      for (int r = 0; r < NR; r++) sx += ar[r] * dx[Rl(r)];
      sx += xI ? dxme : 0.0;
#pragma unroll
      for (int c = 0; c < 2; c++) sx += br[c] * du[c];
      *((k < N - 1 && lane < NX) ? dxn + lane : fdummy) = sx;
    }
  }
}

// SLOTS: the images are where ric_chain_slack_backward left them, in the instance's slots, and the step goes there too
template <class C, int LPI, bool SLOTS, class RP, class SP>
__device__ __forceinline__ void ric_rollout(const RicCtx<C, LPI> &ctx, const RP *const rb, gdouble *const kpb, const int kps,
                                            const StepOut<SP> so, const ldouble *const slots, const ldouble *const limg,
                                            RicStamps &rst) {
  constexpr int NQ = C::NQ, NX = C::NX, NS = C::NS, NV = C::NV, NW = C::NW, GS = FusedSlots<C>::GS;
  constexpr bool DD = RicCtx<C, LPI>::DD;
  constexpr int NP2 = RicCtx<C, LPI>::NP2, KPW = RicCtx<C, LPI>::KPW, KPL = RicCtx<C, LPI>::KPL, TPL = RicCtx<C, LPI>::TPL;
  constexpr bool LIMG = !SLOTS && RicLds<C, LPI>::LIMG;
  constexpr int LCAP = LIMG ? RicLds<C, LPI>::IMG_SLOTS : 0;   // stages 1 .. LCAP keep their image in LDS (limg)
  constexpr size_t sstr = SLOTS ? (size_t)GS : (size_t)C::RS;   // stage stride of the records
  const int N = ctx.N, lane = ctx.lane;
  const double h = ctx.h, h2 = ctx.h2;
  ldouble *const img = ctx.img, *const sAB = ctx.sAB, *const sdx = ctx.sdx, *const sdw = ctx.sdw;
  ldouble *const gdummy = ctx.sT + lane % RicLds<C, LPI>::TW;   // idle lanes store to a word of the unused T area
  const int glr = lane < NX ? lane : 0;
  // ---- forward rollout + costates nu+_k = P_k dx_k + p_k ------------------------------------------
  // the image of stage 0 is still in LDS; later stages come back from the gain record (one request each)
  WSYNC();
  if (lane < NX) sdx[lane] = 0.0;
  // Gain images from global memory: FD stages in flight.  (One stage ahead was not enough: a stage of the rollout is
  // ~600 cycles of work and an image takes several thousand cycles to come back from the Infinity Cache -- the gain
  // records of a launch, 39 MB for 1024 arms, do not fit the L2 -- so that the arm's rollout was 3.4 k cycles per
  // stage, 40 % of its recursion: tests/tools/dev_ric_stamps.py.)  The stage loop is unrolled FD times so that the
  // buffer index is static; requests beyond the horizon are clamped, not skipped.
  constexpr int FD = SLOTS ? 1 : 4;
  double fvq[FD][KPL];
  auto fetch_fwd = [&](int k, double (&fv)[KPL]) __attribute__((always_inline)) {
    const int kk = k < N ? k : N - 1;
#pragma unroll
    for (int u = 0; u < KPL; u++) {
      const int e = lane + LPI * u;
      fv[u] = kpb[(size_t)kk * kps + (e < KPW ? e : 0)];
    }
  };
  if constexpr (!SLOTS) {
#pragma unroll
    for (int d = 0; d < FD; d++) fetch_fwd(LCAP + 1 + d, fvq[d]);
  }
  // (straight-line stages as in the backward pass: clamped per-lane rows, reads before the first use, idle lanes
  //  store to gdummy; the two stores of the step to global memory stay predicated)
  const bool fisw = lane < NW, fact = lane < NW + NX;
  const int fi = fisw ? lane : (fact ? lane - NW : 0);
  const int foff = fisw ? (NW * NX + lane) : (NW * NX + NW + NP2 + fi);
  int frow[NX];
#pragma unroll
  for (int j = 0; j < NX; j++) frow[j] = fisw ? (lane * NX + j) : (NW * NX + NW + ric_tri<NX>(fi, j));
  ldouble *const fdwdst = fisw ? sdw + lane : gdummy;
  ldouble *fimg[KPL];
#pragma unroll
  for (int u = 0; u < KPL; u++) fimg[u] = lane + LPI * u < KPW ? img + lane + LPI * u : gdummy;
  const bool fisq = glr < NQ;
  auto fwd_stage = [&](const int k, double (&fv)[KPL], const bool from_mem) __attribute__((always_inline)) {
    // image of this stage: stage 0's is still in the work area; later ones are read where the backward pass left
    // them (SLOTS; limg for stages 1 .. LCAP), or come back from the gain record (copied into the work area)
    const ldouble *const im = SLOTS ? slots + (size_t)k * GS
                              : ((LIMG && !from_mem && k > 0) ? limg + (size_t)(k - 1) * KPW : img);
    if constexpr (!SLOTS) {
      if (from_mem) {
#pragma unroll
        for (int u = 0; u < KPL; u++) *fimg[u] = fv[u];
        fetch_fwd(k + FD, fv);   // (the buffer is free again: the image of stage k + FD takes its place)
      }
    }
    if constexpr (DD) {
      if (k < N - 1) {   // [A|B] of stage k straight from its record (diff-drive only)
#pragma unroll
        for (int u = 0; u < TPL; u++) {
          const int e = lane + LPI * u;
          const double v = rb[(size_t)k * sstr + ctx.abp[u]] + ctx.abc[u];
          if (e < NX * NV) sAB[e] = v;
        }
      }
    }
    WSYNC();
    rst(5);
    // (the defect of the stage, read before the step of the stage may overwrite it: SLOTS)
    const double rcv = im[NW * NX + NW + NP2 + NX + glr];
    // dw = kff + K dx (lanes < NW) and nu+ = p + P dx (the next NX lanes) as ONE instruction stream: both
    // are "offset + row . dx" over the image, only the per-lane addresses differ (LDS instruction count
    // is what bounds this kernel when the whole batch iterates)
    double dxv[NX], rowv[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) { dxv[j] = sdx[j]; rowv[j] = im[frow[j]]; }
    double sacc = im[foff];
    const double dxi = sdx[fi < NX ? fi : 0];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NX; j++) sacc += rowv[j] * dxv[j];
    *fdwdst = sacc;
    const double dzv = fisw ? sacc : dxi;
    // dz of the stage in one request: lanes < NW hold dw (slots NX..), the next NX lanes dx (slots 0..)
    if constexpr (SLOTS) {
      if (fact && !fisw && k >= 1) so.nunew[(size_t)fi * so.SS + (size_t)k * so.KS] = sacc;
      if (fact) so.dz[(size_t)(fisw ? NX + lane : lane - NW) * so.SS + (size_t)k * so.KS] = dzv;
    } else {
      // (unconditional stores, idle lanes to the spare word of the stage's gain record: behind a predicated store the
      //  compiler no longer knows how many requests are in flight and waits for ALL of them -- the images of the next
      //  stages included -- before it touches the oldest)
      SP *const sink = kpb + (size_t)k * kps + KPW;
      *((fact && !fisw && k >= 1) ? so.nunew + (size_t)fi * so.SS + (size_t)k * so.KS : sink) = sacc;
      *(fact ? so.dz + (size_t)(fisw ? NX + lane : lane - NW) * so.SS + (size_t)k * so.KS : sink) = dzv;
    }
    WSYNC();
    double dxn = 0.0;
    if constexpr (!DD) {
      // holonomic chain, closed form of rc + [A|B][dx; dw] (same order of the non-zero terms as the dense
      // product): q rows dx_i + h dx_{n+i} + h2 dw_i, v rows dx_i + h dw_{i-n}
      const double d0 = sdx[glr], d1 = sdx[fisq ? NQ + glr : glr], w0 = sdw[NS + (fisq ? glr : glr - NQ)];
      __builtin_amdgcn_sched_barrier(0);
      double sx = rcv;
      sx += d0;
      sx += (fisq ? h : 0.0) * d1;
      sx += (fisq ? h2 : h) * w0;
      dxn = sx;
    } else {
      double sx = rcv;
#pragma unroll
      for (int j = 0; j < NX; j++) sx += sAB[glr * NV + j] * sdx[j];
#pragma unroll
      for (int j = 0; j < NW; j++) sx += sAB[glr * NV + NX + j] * sdw[j];
      dxn = sx;
    }
    // (all lanes have issued their reads of sdx before this store: same wavefront, program order)
    *((k < N - 1 && lane < NX) ? sdx + lane : gdummy) = dxn;
    // (next stage's barrier orders this write before the reads)
    rst(6);
  };
  // stage 0 and the stages whose image stayed in LDS, then the stages from the gain record: stage LCAP + 1 + d (+ FD,
  // + 2 FD ...) waits in buffer d
  for (int k = 0; k < N && k <= LCAP; k++) fwd_stage(k, fvq[0], false);
  if constexpr (!SLOTS) {
    for (int k0 = LCAP + 1; k0 < N; k0 += FD) {
#pragma unroll
      for (int d = 0; d < FD; d++) {
        if (k0 + d < N) fwd_stage(k0 + d, fvq[d], true);   // (uniform branch: N and k0 are wave-uniform)
      }
    }
  } else {
    for (int k = 1; k < N; k++) fwd_stage(k, fvq[0], false);
  }
  rst.flush(lane);
}

// Block-tridiagonal Riccati recursion of one instance, LPI lanes.  img: the instance's LDS row (RicLds::LDSW
// doubles); rb: its stage records (stage 0, stride C::RS; global memory or LDS); kpb: its gain records (stride
// kps, global memory).  Returns false when a stage's control block is not positive definite.
// SLOTS: rb == slots (records), gains go to the slots as well (kpb unused); OWNER: the fused kernel (records and gains in
// global memory); SP: where the step goes; limg (RicLds::LIMG): RicLds::IMG_SLOTS gain images of KPW doubles in LDS,
// stages 1 .. IMG_SLOTS; lcap_rt >= 0: number of those slots (the fused arm kernel; otherwise RicLds::IMG_SLOTS).
template <class C, int LPI, bool SLOTS = false, class RP = gdouble, bool OWNER = false, class SP = RP>
__device__ __forceinline__ bool riccati_recursion(const int N, const double dt, const double mu, const double cw, const int lane,
                                                  ldouble *const img, const RP *const rb, gdouble *const kpb,
                                                  const int kps, const StepOut<SP> so, ldouble *const slots = nullptr,
                                                  ldouble *const limg = nullptr, const int lcap_rt = -1) {
  constexpr bool DD = (C::ROBOT == RMPC_ROBOT_DIFFDRIVE);
  static_assert(!(SLOTS && DD), "records in the LDS slots: holonomic chains only");
  const RicCtx<C, LPI> ctx(N, dt, mu, cw, lane, img);
  for (int e = lane; e < C::NX * C::NX; e += LPI) ctx.sP[e] = 0.0;   // P = 0, p = 0 behind the last stage
  if (lane < C::NX) ctx.sp[lane] = 0.0;
  if constexpr (SLOTS && C::NS == 0) {
    return ric_point_robot(ctx, slots, so);
  } else if constexpr (RicLds<C, LPI>::ARMB) {
    return ric_arm_block(ctx, rb, kpb, kps, so, limg, lcap_rt);
  } else {
    RicStamps rst;
    bool ok;
    if constexpr (SLOTS) ok = ric_chain_slack_backward(ctx, slots, rst);
    else if constexpr (DD && OWNER) ok = ric_dd_backward(ctx, rb, kpb, kps);
    else ok = ric_backward(ctx, rb, kpb, kps, limg, rst);
    if (!ok) return false;
    if constexpr (DD && OWNER) ric_dd_rollout(ctx, rb, kpb, kps, so);
    else ric_rollout<C, LPI, SLOTS>(ctx, rb, kpb, kps, so, slots, limg, rst);
    return true;
  }
}
