// rmpc_ric_common.hpp -- what every path of the Riccati recursion shares: the small linear algebra of the control block
// (chol_factor, tri_forward, tri_backward, chol_solve), WSYNC, lds_requests_done, StepOut, the DPP gathers and sums,
// stage_ptr, RicStamps, the layout of the instance's LDS row (RicLds, FusedSlots), ric_tri, the closed-form [A|B] of
// the holonomic chain (ChainVar) and the per-lane constants of RicCtx.  Part of rmpc_riccati.hpp (included there,
// inside namespace rmpc, ahead of the paths); k_riccati_lane (rmpc_pass_riccati.hpp) uses the helpers as well.

// Cholesky factor L of the control block in registers, with the reciprocals of its diagonal (no divisions on the chain),
// from the lower triangle of the NW x NW block of q that begins at (O, O).  Clears ok when a pivot is not positive.
// (The flag is the caller's, not a return value: a stage loop then carries the one and-chain it carried with the loop
// written out, and compiles to the same registers.)
template <int NW, int O = 0, int M>
__device__ __forceinline__ void chol_factor(const double (&q)[M][M], double (&L)[NW][NW], double (&invd)[NW], bool &ok) {
  static_assert(O + NW <= M, "chol_factor: the block lies inside q");
#pragma unroll
  for (int j = 0; j < NW; j++) {
    double dg = q[O + j][O + j];
#pragma unroll
    for (int l = 0; l < j; l++) dg -= L[j][l] * L[j][l];
    if (!(dg > 0.0)) ok = false;
    // 1/sqrt(dg): hardware estimate + two Newton steps (full double precision), then sqrt = dg * rsqrt
    double inv = __builtin_amdgcn_rsq(dg);
    inv = inv * (1.5 - 0.5 * dg * inv * inv);
    inv = inv * (1.5 - 0.5 * dg * inv * inv);
    L[j][j] = dg * inv;
    invd[j] = inv;
#pragma unroll
    for (int i = j + 1; i < NW; i++) {
      double s = q[O + i][O + j];
#pragma unroll
      for (int l = 0; l < j; l++) s -= L[i][l] * L[j][l];
      L[i][j] = s * inv;
    }
  }
}

// v <- L^-1 v
template <int NW>
__device__ __forceinline__ void tri_forward(const double (&L)[NW][NW], const double (&invd)[NW], double (&v)[NW]) {
#pragma unroll
  for (int i = 0; i < NW; i++) {
    double s = v[i];
#pragma unroll
    for (int l = 0; l < i; l++) s -= L[i][l] * v[l];
    v[i] = s * invd[i];
  }
}

// v <- L^-T v
template <int NW>
__device__ __forceinline__ void tri_backward(const double (&L)[NW][NW], const double (&invd)[NW], double (&v)[NW]) {
#pragma unroll
  for (int i = NW - 1; i >= 0; i--) {
    double s = v[i];
#pragma unroll
    for (int l = i + 1; l < NW; l++) s -= L[l][i] * v[l];
    v[i] = s * invd[i];
  }
}

// L L^T x = v
template <int NW>
__device__ __forceinline__ void chol_solve(const double (&L)[NW][NW], const double (&invd)[NW], double (&v)[NW]) {
  tri_forward<NW>(L, invd, v);
  tri_backward<NW>(L, invd, v);
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

// [A | B] of the holonomic chain in closed form: A = [I hI; 0 I], B = [h2 I; h I] on the u columns.  The row of
// [A | B]^T that belongs to a variable of joint j is f1 times block row q+_j plus f2 times block row v+_j: (1, 0) for q_j,
// (h, 1) for v_j, (h2, h) for u_j.
struct ChainRow {
  double f1, f2;
};
__device__ __forceinline__ ChainRow chain_row(const int kind, const double h, const double h2) {
  return {kind == 0 ? 1.0 : (kind == 1 ? h : h2), kind == 0 ? 0.0 : (kind == 1 ? 1.0 : h)};
}
// Variable i of a stage of configuration C (q | v | slack | u): its kind (0 q, 1 v, 2 u, 3 slack), its joint and its row
// factors.  The slack has no joint (negative here) and no row in [A | B] (its factors are not zero here): the caller
// leaves its entries out, or forces block position and factors to zero.  (joint and row are formed where they are
// asked for, so a caller's per-lane constants keep the order it sets them in.)
template <class C>
struct ChainVar {
  int i, kind;
  __device__ __forceinline__ ChainVar(const int i_)
      : i(i_), kind(i_ < C::NQ ? 0 : (i_ < C::NX ? 1 : (i_ >= C::NX + C::NS ? 2 : 3))) {}
  __device__ __forceinline__ int joint() const { return kind == 0 ? i : (kind == 1 ? i - C::NQ : i - C::NX - C::NS); }
  __device__ __forceinline__ ChainRow row(const double h, const double h2) const { return chain_row(kind, h, h2); }
};

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
          const int s = ric_tri<NQ>(i, j);
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
