// rmpc_ric_dense.hpp -- ric_backward, ric_rollout: the generic dense form of the recursion (pass kernels, every model
// without a path of its own) and the rollout it shares with ric_chain_slack_backward.  Part of rmpc_riccati.hpp (included
// there, inside namespace rmpc); needs rmpc_ric_common.hpp.

// ---- pass kernels: the backward pass in the generic dense form ----------------------------------------------------
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
    // row / column kind: 0 = q, 1 = v, 2 = u, 3 = slack (no contribution).  (Kind and joint as ChainVar forms them,
    // written out: through the helper the grouped kernels of the small chains spill other numbers of scalar registers)
    const int ki = i < NQ ? 0 : (i < NX ? 1 : (i >= NX + NS ? 2 : 3));
    const int kj = j < NQ ? 0 : (j < NX ? 1 : (j >= NX + NS ? 2 : 3));
    gon[u] = ok && ki != 3 && kj != 3;
    const int ii = !gon[u] ? 0 : (ki == 0 ? i : (ki == 1 ? i - NQ : i - NX - NS));
    const int jj = !gon[u] ? 0 : (kj == 0 ? j : (kj == 1 ? j - NQ : j - NX - NS));
    go11[u] = ii * NX + jj;
    // left factor: the row's kind picks the combination of the two block rows; right factor: the column's likewise
    gl1[u] = chain_row(ki, h, h2).f1; gl2[u] = chain_row(ki, h, h2).f2;
    gc1[u] = chain_row(kj, h, h2).f1; gc2[u] = chain_row(kj, h, h2).f2;
    gqdst[u] = ok ? sQ + e : gdummy;
  }
  const int glr = lane < NX ? lane : 0, glv = lane < NV ? lane : 0;
  ldouble *const gsrc = lane < NX ? src + lane : gdummy, *const gpcdst = lane < NX ? sPc + lane : gdummy;
  ldouble *const gsqdst = lane < NV ? sq + lane : gdummy;
  const int gkq = glv < NQ ? 0 : (glv < NX ? 1 : (glv >= NX + NS ? 2 : 3));
  const bool gqon = lane < NV && gkq != 3;
  const int giq = !gqon ? 0 : (gkq == 0 ? glv : (gkq == 1 ? glv - NQ : glv - NX - NS));
  const double gl1q = chain_row(gkq, h, h2).f1, gl2q = chain_row(gkq, h, h2).f2;
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
      // to gdummy) -- as for the fused kernel's paths; same arithmetic per entry.
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
    chol_factor<NW>(qw, L, invd, chol_ok);
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
