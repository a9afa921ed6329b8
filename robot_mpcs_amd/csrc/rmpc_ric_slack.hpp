// rmpc_ric_slack.hpp -- ric_chain_slack_backward: the backward pass of the fused kernel for the chains with the slack
// variable (its rollout is ric_rollout, rmpc_ric_dense.hpp).  Part of rmpc_riccati.hpp (included there, inside namespace
// rmpc); needs rmpc_ric_common.hpp.

// ---- fused kernel, holonomic chain: the backward pass on the instance's LDS slots ---------------------
// Same arithmetic per entry as the generic path (ric_backward), organised for a wavefront that runs alone on its
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
    const ChainVar<C> vi(i), vj(j);
    const bool on = vi.kind != 3 && vj.kind != 3;   // (an entry that involves the slack: left factors zero, block (0, 0))
    const int ii = !on ? 0 : vi.joint(), jj = !on ? 0 : vj.joint();
    o11[u] = ii * NX + jj;
    const ChainRow fl = vi.row(h, h2), fc = vj.row(h, h2);
    l1[u] = !on ? 0.0 : fl.f1; l2[u] = !on ? 0.0 : fl.f2;
    c1[u] = fc.f1; c2[u] = fc.f2;
  }
  // the lane's gradient entry (lanes < NV)
  const int lv = lane < NV ? lane : 0;
  const ChainVar<C> vq(lv);
  const int iq = vq.kind == 3 ? 0 : vq.joint();
  const double l1q = vq.kind == 3 ? 0.0 : vq.row(h, h2).f1, l2q = vq.kind == 3 ? 0.0 : vq.row(h, h2).f2;
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
    chol_factor<NW>(qw, L, invd, chol_ok);
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
