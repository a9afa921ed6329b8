// rmpc_pass_riccati.hpp -- the pass kernels around the recursion: k_riccati (a wavefront, or half of one, per instance)
// and k_riccati_lane (a lane per instance).  Part of rmpc_kernels.hip (included there, inside namespace rmpc); needs
// rmpc_inst.hpp and rmpc_riccati.hpp (riccati_recursion; the lane kernel takes the small linear algebra, ric_tri and the
// chain's [A|B] from rmpc_ric_common.hpp).

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
  for (int k = lane; k < N; k += LPI) reduced_add(r, W, k, b, first != 0);
  {
    // (all quantities through the xor tree together, step by step: 6 exchange rounds instead of 11 x 6 dependent ones;
    //  the same trees as wave_sum / wave_max / wave_min.  The early returns above are uniform over the LPI lanes of an
    //  instance, so whole instances arrive here: the wavefront, or in the grouped regime one or both of its halves --
    //  what the vector-move exchanges need)
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
  // what of the instance state stays live across the recursion: mu, and the two words the rule after it reads
  const double mu = s.mu, theta_c = s.theta_c;
  const int curv_back = s.curv_back;
  __shared__ double lds[IPB * IPW][RicLds<C, LPI>::LDSW];
  constexpr int IMGW = RicLds<C, LPI>::IMG_SLOTS * RicLds<C, LPI>::KPW;
  __shared__ double limg[IMGW > 0 ? IMGW : 1];   // (the arms: gain images of the first IMG_SLOTS stages, one-wavefront blocks)
  static_assert(IMGW == 0 || IPB * IPW == 1, "image slots: one instance per block");
  StepOut<gdouble> so;
  so.dz = (gdouble *)(W.dz + b); so.nunew = (gdouble *)(W.nunew + b); so.SS = (size_t)N * W.Bp; so.KS = (size_t)W.Bp;
  const double cw = usec ? (C::CSCALE ? theta_c : 1.0) : 0.0;
  const bool chol_ok = riccati_recursion<C, LPI, false, gdouble>(M.N, M.dt, mu, cw, lane, (ldouble *)lds[wv],
                                                                 (const gdouble *)(W.R + (size_t)b * N * C::RS),
                                                                 (gdouble *)(W.KP + (size_t)b * N * W.kps), W.kps, so,
                                                                 nullptr, (ldouble *)limg);
  if (L0) store_after_recursion<C>(W, b, chol_ok, usec, theta_c, curv_back);
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
  for (int k = 0; k < N; k++) reduced_add(r, W, k, b, first != 0);
  Inst s;
  inst_load(s, W, b);
  bool usec = false;
  const bool recurse = inst_decide<C>(M, s, r, first != 0, usec);
  inst_store(s, W, b);
  if (!recurse) return;
  const double mu = s.mu, theta_c = s.theta_c, cwt = usec ? (C::CSCALE ? theta_c : 1.0) : 0.0;
  const int curv_back = s.curv_back;
  const double h = M.dt, h2 = 0.5 * M.dt * M.dt;
  constexpr int NP2 = NX * (NX + 1) / 2;
  constexpr int OFF_KFF = NW * NX, OFF_PT = NW * NX + NW, OFF_P = OFF_PT + NP2, OFF_RC = OFF_P + NX;
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
          const int t = ric_tri<NQ>(i, j);
          v = rec[C::R_Q + t] - cwt * (C::CURV ? (double)rec[C::R_C + t] : 0.0);
        } else if (lo == hi) {
          v = rec[C::R_DG + (lo - NQ)];
        } else if (NS > 0 && lo == NX) {
          v = rec[C::R_CS + hi];
        } else if (NS > 0 && hi == NX) {
          v = rec[C::R_CS + lo];
        }
        const ChainVar<C> vi(i), vj(j);
        if (vi.kind != 3 && vj.kind != 3) {
          const int ii = vi.joint(), jj = vj.joint();
          const ChainRow l = vi.row(h, h2), c = vj.row(h, h2);
          const double add = l.f1 * (c.f1 * P[ii][jj] + c.f2 * P[ii][NQ + jj]) + l.f2 * (c.f1 * P[NQ + ii][jj] + c.f2 * P[NQ + ii][NQ + jj]);
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
      const ChainVar<C> vi(i);
      if (vi.kind != 3) {
        const int ii = vi.joint();
        const ChainRow l = vi.row(h, h2);
        const double add = l.f1 * Pc[ii] + l.f2 * Pc[NQ + ii];
        v += rec_cost ? add : 0.0;
      }
      q[i] = v;
    }
    // ---- Cholesky of Qww, gains ----------------------------------------------------------------------------------
    double L[NW][NW], invd[NW];
    chol_factor<NW, NX>(Q, L, invd, chol_ok);
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
      for (int j = i; j < NX; j++) kpk[OFF_PT + ric_tri<NX>(i, j)] = P[i][j];
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
          for (int j = 0; j < NX; j++) sacc += im[OFF_PT + ric_tri<NX>(i, j)] * dx[j];
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
  store_after_recursion<C>(W, b, chol_ok, usec, theta_c, curv_back);
}
