// rmpc_step_debug.hpp -- test aid behind rmpc_debug_step / rmpc_debug_step_curv: one first sweep and one Riccati
// recursion of the fused kernels, stopped there.  The kernels below call the SAME phase functions as k_fused /
// k_fused_arm (the first-pass copy of the sweep call, then fused_recursion_lds / fused_recursion_mem /
// arm_recursion_call), with the same dealing of stages to lanes, the same LDS carving and the same image-slot count,
// and copy out what the recursion consumed (the stage records, before the recursion turns the LDS slots into gain
// images) and what it left (dz | nu+).  use_curv: what the sweep takes for DevModel::use_curv (0: the records carry no
// curvature terms); cw: the weight the recursion gives the records' curvature entries (Q = r0 - cw r1; 0: the
// Gauss-Newton blocks, so that the records' Q, q0, q1, rc are exactly what it consumed).  For the pass kernels:
// k_riccati_step_debug, the recursion call of k_riccati's one-wavefront blocks at a given weight (k_riccati takes its
// weight from the instance's state), and k_lane_weight for k_riccati_lane, whose recursion is no function of its own.
// Included by rmpc_variants.hip only; k_fused, k_fused_arm and the pass kernels are not touched.
#pragma once

namespace rmpc {

// k_fused: a half-wavefront per instance, lane = stage.  rec [B][N][C::RS], dz [B][N][NV], nu [B][N][NX], mu [B], ok [B]
template <class C, bool REC_LDS, class V>
__global__ __launch_bounds__(64, 1) __attribute__((amdgpu_waves_per_eu(1, 1), disable_tail_calls))
void k_fused_step_debug(const DevModel M, const DevTables *__restrict__ Tp, const FusedWs F, const int B,
                        const double *__restrict__ xinit, const double *__restrict__ x0, const double *__restrict__ params,
                        const int warm, const int use_curv, const double cw, double *__restrict__ out_rec,
                        double *__restrict__ out_dz, double *__restrict__ out_nu, double *__restrict__ out_mu,
                        int *__restrict__ out_ok) {
  constexpr int LPI = kFusedStages, IPW = 2;
  constexpr int NX = C::NX, NV = C::NV;
  using VC = typename std::conditional<V::SPEC, V, GView>::type;
  const int half = threadIdx.x / LPI;
  const int k = threadIdx.x & (LPI - 1);
  const int N = M.N;
  const bool stage = k < N;
  constexpr int LW = RicLds<C, LPI>::LDSW;
  constexpr int GS = FusedSlots<C>::GS;
  constexpr int DZ_OFF = FusedSlots<C>::DZ_OFF;
  constexpr int RECW = REC_LDS ? kFusedStages * GS : 0;
  __shared__ double lds[IPW * (LW + RECW)];
  ldouble *const work = (ldouble *)lds + half * (LW + RECW);
  ldouble *const slots = work + LW;
  __shared__ SweepStepOut sres[IPW];
  const size_t S = kFusedStages;
  const int pos = blockIdx.x * IPW + half;
  const bool act = pos < B;
  const size_t b = (size_t)(act ? pos : B - 1);   // (an idle half: addresses stay legal, nothing is written)
  const FusedWs *const Fp = (const FusedWs *)(Tp + 1);
  double mu = M.mu0;
  // prologue of k_fused: ABI rows of this stage -> the instance's block (x_1 := xinit)
  if (act) {
    const FusedPtrs P0 = fused_ptrs(F, b);
    if (stage) {
      const double *zr = x0 + (b * N + k) * NV;
      for (int j = 0; j < NV; j++) {
        double v = zr[j];
        if (k == 0 && j < NX) v = xinit[b * NX + j];
        P0.pz[0][j * S + k] = v;
      }
      if constexpr (REC_LDS) {
        for (int j = 0; j < NV + NX; j++) slots[k * GS + DZ_OFF + j] = 0.0;
      }
      const double *pr = params + (b * N + k) * M.npar;
      for (int j = 0; j < M.npar; j++) P0.pp[j * S + k] = pr[j];
    }
    if (warm) mu = warm_mu(F.wmu[b], M.mu0);
  }
  GSYNC();
  // ---- first sweep: the copy of the call k_fused makes on the first pass of an instance ----
  constexpr bool MERGE2 = V::SPEC && REC_LDS;
  if constexpr (MERGE2) {
    __attribute__((address_space(3))) SweepStepOut *const so = (__attribute__((address_space(3))) SweepStepOut *)&sres[half];
    fused_sweep_step_call<C, V, 1>(so, Fp, M.N, M.dt, use_curv, b, 0, k, slots, act && stage, true, false, 0, 1.0, 1.0, 0.0, mu, warm);
  } else {
    if (act && stage) (void)fused_sweep_call<C, VC, 1, REC_LDS>(Fp, M.N, M.dt, use_curv, b, 0, k, slots, true, 0.0, 0.0, mu, warm);
  }
  GSYNC();
  // the records as the recursion is about to read them
  if (act && stage) {
    double *const ro = out_rec + (b * N + k) * C::RS;
    if constexpr (REC_LDS) {
      for (int j = 0; j < C::RW; j++) ro[j] = slots[k * GS + j];
    } else {
      const gdouble *const ri = (const gdouble *)F.R + (b * (size_t)N + k) * C::RS;
      for (int j = 0; j < C::RW; j++) ro[j] = ri[j];
    }
  }
  GSYNC();
  // ---- recursion: Q = r0 - cw r1 ----
  bool ok = true;
  if (act) {
    if constexpr (REC_LDS) {
      StepOut<ldouble> so;
      so.dz = slots + DZ_OFF; so.nunew = slots + DZ_OFF + NV; so.SS = 1; so.KS = GS;
      ok = fused_recursion_lds<C>(M.N, M.dt, mu, cw, k, work, slots, so);
    } else {
      const FusedPtrs Pr = fused_ptrs(F, b);
      StepOut<gdouble> so;
      so.dz = Pr.pdz; so.nunew = Pr.pnn; so.SS = S; so.KS = 1;
      ok = fused_recursion_mem<C>(M.N, M.dt, mu, cw, k, work, (gdouble *)F.R + b * (size_t)N * C::RS,
                                  (gdouble *)F.KP + b * (size_t)N * F.kps, F.kps, so);
    }
  }
  GSYNC();   // dz, nunew
  if (act && stage) {
    double *const dzo = out_dz + (b * N + k) * NV, *const nuo = out_nu + (b * N + k) * NX;
    if constexpr (REC_LDS) {
      for (int j = 0; j < NV; j++) dzo[j] = slots[k * GS + DZ_OFF + j];
      for (int j = 0; j < NX; j++) nuo[j] = slots[k * GS + DZ_OFF + NV + j];
    } else {
      const FusedPtrs Pr = fused_ptrs(F, b);
      for (int j = 0; j < NV; j++) dzo[j] = Pr.pdz[j * S + k];
      for (int j = 0; j < NX; j++) nuo[j] = Pr.pnn[j * S + k];
    }
  }
  if (act && k == 0) { out_mu[b] = mu; out_ok[b] = ok ? 1 : 0; }
}

// k_fused_arm: a wavefront per instance, a stage per P lanes.  rec [B][N][C::RS] is read from the instance's record
// slots by the host (the arms' records stay in global memory: nothing overwrites them).  The arms' sweep reads use_curv
// from the instance block (always the model's); usec: the recursion's weight is 1 (true) or 0.
template <class C, int P>
__global__ __launch_bounds__(64, 1) __attribute__((amdgpu_waves_per_eu(1, 1), disable_tail_calls))
void k_fused_arm_step_debug(const DevModel M, const DevTables *__restrict__ Tp, const FusedWs F, const int B,
                            const double *__restrict__ xinit, const double *__restrict__ x0,
                            const double *__restrict__ params, const int warm, const bool usec,
                            double *__restrict__ out_rec, double *__restrict__ out_dz, double *__restrict__ out_nu,
                            double *__restrict__ out_mu, int *__restrict__ out_ok) {
  constexpr int NX = C::NX, NV = C::NV, SW = ArmLds<C>::SW;
  const int lane = threadIdx.x;
  const int N = M.N;
  extern __shared__ double lds_dyn[];
  ldouble *const work = (ldouble *)lds_dyn;
  ldouble *const lstep = work + ArmLds<C>::step_off();
  ldouble *const hand = work + ArmLds<C>::hand_off(N);
  ldouble *const limg = work + ArmLds<C>::img_off(N);
  const int lcap = ArmLds<C>::img_slots(N);
  __attribute__((address_space(3))) ArmSweepOut *const sres = (__attribute__((address_space(3))) ArmSweepOut *)hand;
  const ArmBlock *const blkp = (const ArmBlock *)(Tp + 1);
  const size_t S = kFusedStages;
  const int ck = lane & 31, ch = lane >> 5;
  const bool cstage = ck < N;
  const size_t b = blockIdx.x;
  if (b >= (size_t)B) return;   // (uniform)
  const FusedPtrs P0 = fused_ptrs(F, b);
  if (cstage) {
    const double *zr = x0 + (b * N + ck) * NV;
    for (int j = ch; j < NV; j += 2) {
      double vz = zr[j];
      if (ck == 0 && j < NX) vz = xinit[b * NX + j];
      P0.pz[0][j * S + ck] = vz;
    }
    const double *pr = params + (b * N + ck) * M.npar;
    for (int j = ch; j < M.npar; j += 2) P0.pp[j * S + ck] = pr[j];
  }
  for (int e = lane; e < N * SW; e += 64) lstep[e] = 0.0;
  const double mu = warm ? warm_mu(F.wmu[b], M.mu0) : M.mu0;
  GSYNC();
  arm_sweep_call<C, P, 1>(sres, blkp, Tp, b, 0, lstep, true, false, 0, 1.0, 1.0, 0.0, mu, warm);
  GSYNC();
  if (cstage) {
    const gdouble *const ri = (const gdouble *)F.R + b * S * C::RS + (size_t)ck * C::RS;
    double *const ro = out_rec + (b * N + ck) * C::RS;
    for (int j = ch; j < C::RW; j += 2) ro[j] = ri[j];
  }
  const bool ok = arm_recursion_call<C>(M.N, M.dt, mu, usec, lane, work, (gdouble *)F.R + b * S * C::RS,
                                        (gdouble *)F.KP + b * (size_t)N * F.kps, F.kps, lstep, limg, lcap);
  GSYNC();   // dz, nu+
  if (cstage) {
    for (int j = ch; j < NV; j += 2) out_dz[(b * N + ck) * NV + j] = lstep[ck * SW + j];
    for (int j = ch; j < NX; j += 2) out_nu[(b * N + ck) * NX + j] = lstep[ck * SW + NV + j];
  }
  if (lane == 0) { out_mu[b] = mu; out_ok[b] = ok ? 1 : 0; }
}

// Pass kernels: the recursion of k_riccati's one-wavefront blocks (the same riccati_recursion instantiation, LDS sizes
// and image slots) on the records k_sweep left, at the weight cw, without the decisions around it: a wavefront per
// instance, mu as k_init stored it.  ok [B]: the recursion's return value; 0 without a recursion for an instance the
// first pass would have stopped (an inverse-barrier row not strictly feasible at the start).
template <class C>
__global__ __launch_bounds__(64, C::RIC_WPE) void k_riccati_step_debug(const DevModel M, const Ws W, const int B, const double cw,
                                                                       int *__restrict__ out_ok) {
  constexpr int LPI = 64;
  const int b = blockIdx.x;
  if (b >= B) return;   // (uniform)
  const int lane = threadIdx.x;
  const int N = M.N;
  double bad = 0.0;
  for (int k = 0; k < N; k++) bad += W.part[IDX(P_BAD, k, b)];
  if (W.status[b] != ST_ACTIVE || bad != 0.0) {
    if (lane == 0) out_ok[b] = 0;
    return;
  }
  const double mu = W.mu[b];
  __shared__ double lds[RicLds<C, LPI>::LDSW];
  constexpr int IMGW = RicLds<C, LPI>::IMG_SLOTS * RicLds<C, LPI>::KPW;
  __shared__ double limg[IMGW > 0 ? IMGW : 1];
  StepOut<gdouble> so;
  so.dz = (gdouble *)(W.dz + b); so.nunew = (gdouble *)(W.nunew + b); so.SS = (size_t)N * W.Bp; so.KS = (size_t)W.Bp;
  const bool ok = riccati_recursion<C, LPI, false, gdouble>(M.N, M.dt, mu, cw, lane, (ldouble *)lds,
                                                            (const gdouble *)(W.R + (size_t)b * N * C::RS),
                                                            (gdouble *)(W.KP + (size_t)b * N * W.kps), W.kps, so,
                                                            nullptr, (ldouble *)limg);
  if (lane == 0) out_ok[b] = ok ? 1 : 0;
}

// k_riccati_lane decides its weight itself (inst_decide: the model uses curvature terms and mu <= kCurvMu; then the
// instance's scale theta_mem where Cfg::CSCALE, else 1).  Sets the scale to cw where that is possible and reports in
// bad [B] whether the first pass of instance b cannot run at the weight cw.
template <class C>
__global__ void k_lane_weight(const DevModel M, const Ws W, const int B, const double cw, int *__restrict__ bad) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const bool nat = (C::CURV || C::DDCURV) && M.use_curv && W.mu[b] <= kCurvMu;
  if (C::CSCALE && nat) W.theta_mem[b] = cw;
  const double w = nat ? (C::CSCALE ? cw : 1.0) : 0.0;
  bad[b] = (M.use_curv && w != cw) ? 1 : 0;   // (a model without terms: every weight is the same recursion)
}

}  // namespace rmpc
