// rmpc_ric_point.hpp -- ric_point_robot: the recursion of the fused kernel for the chains without slack, n <= 3, backward
// pass and rollout.  Part of rmpc_riccati.hpp (included there, inside namespace rmpc); needs rmpc_ric_common.hpp.

// ---- fused kernel, holonomic chain without slack, n <= 3 (the point robot): Schur-complement form on the slots --------
// Round 4.  At four wavefronts per CU the recursion of k_fused is bound by the LDS: the gain form
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
  const int tq = ric_tri<n>(ii, jj);
  const int jme = gj == 0 ? ii : (gj == 1 ? n + ii : (gj == 2 ? 2 * n + ii : 0));   // gradient entry of lanes gj <= 2
  const ChainRow gc = chain_row(gj, h, h2);   // (q_i, v_i, u_i in lanes gj = 0, 1, 2)
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
    const double gme = (rn[6] - mu * rn[7]) + (gc.f1 * g1 + gc.f2 * g2);   // gradient entry q_i / v_i / u_i (gj = 0, 1, 2)
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
      chol_factor<NW>(qw, L, invd, chol_ok);
      tri_forward<NW>(L, invd, colv);   // (in place: colv is the lane's column of Y from here on)
#pragma unroll
      for (int i = 0; i < NW; i++) dY[i * ystr] = colv[i];
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
      tri_backward<NW>(L, invd, colv);
#pragma unroll
      for (int i = 0; i < NW; i++) *stage_ptr(wK[i], strK, k) = -colv[i];
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
