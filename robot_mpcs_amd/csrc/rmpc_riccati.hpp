// rmpc_riccati.hpp -- block-tridiagonal Riccati recursion of one instance, the Riccati step of every kernel family
// (k_riccati, k_fused, k_fused_arm).  Part of rmpc_kernels.hip (included there, inside namespace rmpc, ahead of the
// kernels); needs rmpc_solver.hpp (the DPP moves dpp_move / dpp_row_bcast are there, beside the reductions' exchanges).
//
// riccati_recursion, below, picks one path per model and kernel at compile time; each path is a function of its own, in
// a header of its own:
//   ric_point_robot           rmpc_ric_point.hpp  fused kernel, chains without slack (n <= 3): Schur form on the LDS slots, with its rollout
//   ric_chain_slack_backward  rmpc_ric_slack.hpp  fused kernel, chains with slack: gain form on the LDS slots       -> ric_rollout
//   ric_dd_backward           rmpc_ric_dd.hpp     fused kernel, diff-drive: records and gains in global memory      -> ric_dd_rollout
//   ric_arm_block             rmpc_ric_arm.hpp    pass and fused arm kernels, n = 5 .. 7 without slack: Schur form + MFMA, with its rollout
//   ric_backward              rmpc_ric_dense.hpp  pass kernels, every other model (generic dense form)               -> ric_rollout
// They share rmpc_ric_common.hpp: the factorisation and substitutions of the control block, the chain's closed-form
// [A|B], the layout of the instance's LDS row (RicLds) and the per-lane constants of RicCtx.

#include "rmpc_ric_common.hpp"
#include "rmpc_ric_point.hpp"
#include "rmpc_ric_slack.hpp"
#include "rmpc_ric_dd.hpp"
#include "rmpc_ric_arm.hpp"
#include "rmpc_ric_dense.hpp"

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
