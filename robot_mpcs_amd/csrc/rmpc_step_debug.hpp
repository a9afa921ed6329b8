// rmpc_step_debug.hpp -- test aid behind rmpc_debug_step: one first sweep and one Riccati recursion of the fused
// kernels, stopped there.  The kernels below call the SAME phase functions as k_fused / k_fused_arm (the first-pass
// copy of the sweep call, then fused_recursion_lds / fused_recursion_mem / arm_recursion_call), with the same dealing
// of stages to lanes, the same LDS carving and the same image-slot count, and copy out what the recursion consumed
// (the stage records, before the recursion turns the LDS slots into gain images) and what it left (dz | nu+).  The
// recursion runs on the Gauss-Newton blocks (curvature weight 0), so that the records' Q, q0, q1, rc are exactly
// what it consumed.  Included by rmpc_variants.hip only; k_fused and k_fused_arm are not touched.
#pragma once

namespace rmpc {

// k_fused: a half-wavefront per instance, lane = stage.  rec [B][N][C::RS], dz [B][N][NV], nu [B][N][NX], mu [B], ok [B]
template <class C, bool REC_LDS, class V>
__global__ __launch_bounds__(64, 1) __attribute__((amdgpu_waves_per_eu(1, 1), disable_tail_calls))
void k_fused_step_debug(const DevModel M, const DevTables *__restrict__ Tp, const FusedWs F, const int B,
                        const double *__restrict__ xinit, const double *__restrict__ x0, const double *__restrict__ params,
                        const int warm, double *__restrict__ out_rec, double *__restrict__ out_dz,
                        double *__restrict__ out_nu, double *__restrict__ out_mu, int *__restrict__ out_ok) {
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
    fused_sweep_step_call<C, V, 1>(so, Fp, M.N, M.dt, 0, b, 0, k, slots, act && stage, true, false, 0, 1.0, 1.0, 0.0, mu, warm);
  } else {
    if (act && stage) (void)fused_sweep_call<C, VC, 1, REC_LDS>(Fp, M.N, M.dt, 0, b, 0, k, slots, true, 0.0, 0.0, mu, warm);
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
  // ---- recursion: Gauss-Newton blocks (cw = 0) ----
  bool ok = true;
  if (act) {
    if constexpr (REC_LDS) {
      StepOut<ldouble> so;
      so.dz = slots + DZ_OFF; so.nunew = slots + DZ_OFF + NV; so.SS = 1; so.KS = GS;
      ok = fused_recursion_lds<C>(M.N, M.dt, mu, 0.0, k, work, slots, so);
    } else {
      const FusedPtrs Pr = fused_ptrs(F, b);
      StepOut<gdouble> so;
      so.dz = Pr.pdz; so.nunew = Pr.pnn; so.SS = S; so.KS = 1;
      ok = fused_recursion_mem<C>(M.N, M.dt, mu, 0.0, k, work, (gdouble *)F.R + b * (size_t)N * C::RS,
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
// slots by the host (the arms' records stay in global memory: nothing overwrites them).
template <class C, int P>
__global__ __launch_bounds__(64, 1) __attribute__((amdgpu_waves_per_eu(1, 1), disable_tail_calls))
void k_fused_arm_step_debug(const DevModel M, const DevTables *__restrict__ Tp, const FusedWs F, const int B,
                            const double *__restrict__ xinit, const double *__restrict__ x0,
                            const double *__restrict__ params, const int warm, double *__restrict__ out_rec,
                            double *__restrict__ out_dz, double *__restrict__ out_nu, double *__restrict__ out_mu,
                            int *__restrict__ out_ok) {
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
  const bool ok = arm_recursion_call<C>(M.N, M.dt, mu, false, lane, work, (gdouble *)F.R + b * S * C::RS,
                                        (gdouble *)F.KP + b * (size_t)N * F.kps, F.kps, lstep, limg, lcap);
  GSYNC();   // dz, nu+
  if (cstage) {
    for (int j = ch; j < NV; j += 2) out_dz[(b * N + ck) * NV + j] = lstep[ck * SW + j];
    for (int j = ch; j < NX; j += 2) out_nu[(b * N + ck) * NX + j] = lstep[ck * SW + NV + j];
  }
  if (lane == 0) { out_mu[b] = mu; out_ok[b] = ok ? 1 : 0; }
}

}  // namespace rmpc
