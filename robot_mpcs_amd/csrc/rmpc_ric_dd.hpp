// rmpc_ric_dd.hpp -- ric_dd_backward, ric_dd_rollout: the recursion of the fused kernel for the diff-drive model.  Part of
// rmpc_riccati.hpp (included there, inside namespace rmpc); needs rmpc_ric_common.hpp.

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
  // blocks that each wait for their own reads (as for the chain's path, ric_chain_slack_backward).
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
      chol_factor<NW>(qw, L, invd, chol_ok);
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
