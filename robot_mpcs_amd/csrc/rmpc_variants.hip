// rmpc_variants.hip -- the kernels of some kernel variants and their entries in the host's variant table
// (VariantOps, rmpc_host.hpp).  __graft_entry__.compile_library compiles this file once per group of variants
// (__graft_entry__.TU_MASKS), in parallel with each other, the host unit rmpc_host.hip and rmpc_world.hip: RMPC_UNIT_VARIANTS is
// the bit mask of the rows of RMPC_VARIANTS this unit builds (bit i = id i; default: all of them).
#include "rmpc_host.hpp"
#include "rmpc_step_debug.hpp"

// One kernel variant per robot family and size: X(id, robot kind, n, ns).  ids 0 .. 5 are the shipped configurations
// (point robot, panda, boxer, each without / with the slack variable); 6 .. 10 further holonomic chains (mpcBase.py:52-55:
// n = fk.n() of whatever URDF chain the YAML names), the sizes the test suite can build from the shipped URDFs
// (tests: chain2, chain4, chain5, chain6), and n = 8 = RMPC_MAX_JOINTS (test: chain8, the panda's chain with one more
// revolute joint).  Another size is one more line here and its bit in one of __graft_entry__.TU_MASKS.
#define RMPC_VARIANTS(X)                                                                                                  \
  X(0, RMPC_ROBOT_CHAIN, 3, 0) X(1, RMPC_ROBOT_CHAIN, 3, 1) X(2, RMPC_ROBOT_CHAIN, 7, 0) X(3, RMPC_ROBOT_CHAIN, 7, 1)    \
  X(4, RMPC_ROBOT_DIFFDRIVE, 3, 0) X(5, RMPC_ROBOT_DIFFDRIVE, 3, 1) X(6, RMPC_ROBOT_CHAIN, 2, 0) X(7, RMPC_ROBOT_CHAIN, 4, 0) \
  X(8, RMPC_ROBOT_CHAIN, 5, 0) X(9, RMPC_ROBOT_CHAIN, 6, 0) X(10, RMPC_ROBOT_CHAIN, 8, 0)
#ifndef RMPC_UNIT_VARIANTS
#define RMPC_UNIT_VARIANTS (~0)
#endif

namespace {

template <class C, class V>
void launch_pass(rmpc_handle *h, const Phase &ph, int first, int pass, hipStream_t st, int which) {
  const int B = ph.B;
  const int lanes = ph.W.Bp * h->M.N;
  if (which == K_SWEEP) hipLaunchKernelGGL((k_sweep<C, V>), dim3((lanes + kSweepBlock - 1) / kSweepBlock), dim3(kSweepBlock), 0, st, h->M, h->d_T, ph.W, B, first,
                                           (first && h->warm_mode && h->have_duals) ? 1 : 0);
  else if (which == K_RICCATI) {
    if constexpr (C::ROBOT == RMPC_ROBOT_CHAIN && C::NQ <= 3) {
      // lane-per-instance recursion for large lists (h->ric_lane: 0 never, 1 from kLaneMin instances on, 2 always)
      if (h->ric_lane == 2 || (h->ric_lane == 1 && B >= kLaneMin)) {
        hipLaunchKernelGGL((k_riccati_lane<C>), dim3((B + 63) / 64), dim3(64), 0, st, h->M, ph.W, B, first);
        h->ric_sel = RMPC_PATH_RIC_LANE;
        return;
      }
    }
    h->ric_sel = (C::IPB > 1 && B >= kGroupedMin) ? RMPC_PATH_RIC_GROUPED : RMPC_PATH_RIC_WAVE;
    if (C::IPB > 1 && B >= kGroupedMin)
    {
      constexpr int per_block = C::IPB * (64 / C::RIC_LPI);   // instances per block
      hipLaunchKernelGGL((k_riccati<C, C::IPB>), dim3((B + per_block - 1) / per_block), dim3(64 * C::IPB), 0, st, h->M, ph.W, B, first, pass);
    }
    const int tail_blocks = (C::IPB == 1 || B < kGroupedMin) ? B : kGroupedMin;
    hipLaunchKernelGGL((k_riccati<C, 1>), dim3(tail_blocks), dim3(64), 0, st, h->M, ph.W, B, first, pass);
  }
  else hipLaunchKernelGGL((k_step<C, V>), dim3((lanes + kSweepBlock - 1) / kSweepBlock), dim3(kSweepBlock), 0, st, h->M, h->d_T, ph.W, B);
}

template <class C>
void launch_difficulty(rmpc_handle *h, int B, const double *d_xinit, const double *d_params, hipStream_t st) {
  hipLaunchKernelGGL((k_difficulty<C>), dim3((B + 63) / 64), dim3(64), 0, st, h->M, h->d_T, B, d_xinit, d_params, h->F.ckey);
}

template <class C, class V>
void launch_fused(rmpc_handle *h, int B, const double *d_xinit, const double *d_x0, const double *d_params, double *d_zout,
                  int *d_exit, int *d_iters, double *d_kkt, double *d_obj, hipStream_t st, int cap, int warm, int use_order) {
  // the grid is the chip (one wavefront per SIMD: __launch_bounds__(64, 1)), the batch is a queue its halves drain
  const int pairs = (B + 1) / 2;
  const int grid = pairs < h->fused_grid ? pairs : h->fused_grid;
  // (save_duals: only a handle in warm-start mode reads the multipliers, mu and the pass counts a solve leaves behind)
  hipLaunchKernelGGL((k_fused<C, C::FUSED_REC_LDS, V>), dim3(grid), dim3(64), 0, st, h->M, h->d_T, h->F, B, d_xinit, d_x0,
                     d_params, d_zout, d_exit, d_iters, d_kkt, d_obj, cap, warm, use_order, h->warm_mode ? 1 : 0);
}

template <class C>
void launch_fused_arm(rmpc_handle *h, int B, const double *d_xinit, const double *d_x0, const double *d_params, double *d_zout,
                      int *d_exit, int *d_iters, double *d_kkt, double *d_obj, hipStream_t st, int cap, int warm, int use_order) {
  // the grid is the chip (one wavefront per SIMD), the batch a queue its wavefronts drain
  const int grid = B < h->fused_grid ? B : h->fused_grid;
  // parts per stage: three when the horizon leaves room for them (3 N <= 64 lanes), else two
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void *)k_fused_arm<C, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, ArmLds<C>::TOTAL * 8);
    (void)hipFuncSetAttribute((const void *)k_fused_arm<C, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, ArmLds<C>::TOTAL * 8);
    attr_set = true;
  }
  if (3 * h->M.N <= 64 && !h->env_arm_two_parts)
    hipLaunchKernelGGL((k_fused_arm<C, 3>), dim3(grid), dim3(64), ArmLds<C>::TOTAL * 8, st, h->M, h->d_T, h->F, B, d_xinit, d_x0,
                       d_params, d_zout, d_exit, d_iters, d_kkt, d_obj, cap, warm, use_order);
  else
    hipLaunchKernelGGL((k_fused_arm<C, 2>), dim3(grid), dim3(64), ArmLds<C>::TOTAL * 8, st, h->M, h->d_T, h->F, B, d_xinit, d_x0,
                       d_params, d_zout, d_exit, d_iters, d_kkt, d_obj, cap, warm, use_order);
}

// rmpc_debug_step on a fused handle: the grid and the parts per stage of launch_fused / launch_fused_arm
template <class C, class V>
void launch_fused_step_debug(rmpc_handle *h, int B, const double *d_xinit, const double *d_x0, const double *d_params, int warm,
                             int use_curv, double cw, double *d_rec, double *d_dz, double *d_nu, double *d_mu, int *d_ok,
                             hipStream_t st) {
  hipLaunchKernelGGL((k_fused_step_debug<C, C::FUSED_REC_LDS, V>), dim3((B + 1) / 2), dim3(64), 0, st, h->M, h->d_T, h->F, B,
                     d_xinit, d_x0, d_params, warm, use_curv, cw, d_rec, d_dz, d_nu, d_mu, d_ok);
}

template <class C>
void launch_fused_arm_step_debug(rmpc_handle *h, int B, const double *d_xinit, const double *d_x0, const double *d_params, int warm,
                                 int use_curv, double cw, double *d_rec, double *d_dz, double *d_nu, double *d_mu, int *d_ok,
                                 hipStream_t st) {
  (void)use_curv;   // (arm_sweep_call reads it from the instance block)
  const bool usec = cw != 0.0;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void *)k_fused_arm_step_debug<C, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, ArmLds<C>::TOTAL * 8);
    (void)hipFuncSetAttribute((const void *)k_fused_arm_step_debug<C, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, ArmLds<C>::TOTAL * 8);
    attr_set = true;
  }
  if (3 * h->M.N <= 64 && !h->env_arm_two_parts)
    hipLaunchKernelGGL((k_fused_arm_step_debug<C, 3>), dim3(B), dim3(64), ArmLds<C>::TOTAL * 8, st, h->M, h->d_T, h->F, B, d_xinit,
                       d_x0, d_params, warm, usec, d_rec, d_dz, d_nu, d_mu, d_ok);
  else
    hipLaunchKernelGGL((k_fused_arm_step_debug<C, 2>), dim3(B), dim3(64), ArmLds<C>::TOTAL * 8, st, h->M, h->d_T, h->F, B, d_xinit,
                       d_x0, d_params, warm, usec, d_rec, d_dz, d_nu, d_mu, d_ok);
}

// rmpc_debug_step_curv on the pass kernels: see VariantOps::pass_step_debug
template <class C, class V>
int launch_pass_step_debug(rmpc_handle *h, const Phase &ph, double cw, int *d_ok, hipStream_t st) {
  const int B = ph.B;
  if constexpr (C::ROBOT == RMPC_ROBOT_CHAIN && C::NQ <= 3) {
    if (h->ric_lane == 2 || (h->ric_lane == 1 && B >= kLaneMin)) {
      hipLaunchKernelGGL((k_lane_weight<C>), dim3((B + 63) / 64), dim3(64), 0, st, h->M, ph.W, B, cw, d_ok);
      launch_pass<C, V>(h, ph, 1, 0, st, K_RICCATI);
      return 1;
    }
  }
  hipLaunchKernelGGL((k_riccati_step_debug<C>), dim3(B), dim3(64), 0, st, h->M, ph.W, B, cw, d_ok);
  return 0;
}

template <class C>
void launch_advance(rmpc_handle *h, int B, const double *d_z_prev, const int *ef, double *d_xinit, double *d_x0, int previous_plan,
                    hipStream_t st) {
  hipLaunchKernelGGL((k_advance<C>), dim3((B + kAdvanceIB - 1) / kAdvanceIB), dim3(256), 0, st, h->M, d_z_prev, d_xinit, d_x0, B,
                     previous_plan, ef);
}

template <class C>
void launch_retarget(rmpc_handle *h, int B, const RetargetDev &R, hipStream_t st) {
  hipLaunchKernelGGL((k_retarget<C>), dim3((B + 255) / 256), dim3(256), 0, st, h->M, h->d_T, B, R);
}

// true when every accessor of the generated view S returns what the runtime tables hold
template <class S>
bool spec_matches(const rmpc_desc &d, const DevModel &M, const DevTables &T) {
  if (S::ROBOT != d.robot || S::NQ != d.n || S::NS != d.ns) return false;
  bool ok = S::nslots() == T.nslots && S::nfkrows() == T.nfkrows;
  for (int i = 0; i < kMaxSlots; i++) ok = ok && S::slot_fa(i) == T.slot_fa[i] && S::slot_fb(i) == T.slot_fb[i];
  for (int i = 0; i <= kMaxSlots; i++) ok = ok && S::slot_row_begin(i) == T.slot_row_begin[i];
  for (int i = 0; i < kMaxFkRows; i++)
    ok = ok && S::fk_row(i) == T.fk_row[i] && S::fk_kind(i) == T.fk_kind[i] && S::fk_obst(i) == T.fk_obst[i] &&
         S::fk_mod(i) == T.fk_mod[i] && S::fk_first(i) == T.fk_first[i] && S::fk_idx(i) == T.fk_idx[i];
  for (int j = 0; j < RMPC_NV_MAX; j++)
    for (int u = 0; u < kVarRows; u++)
      ok = ok && S::v_row(j, u) == T.v_row[j][u] && S::v_sgn(j, u) == T.v_sgn[j][u] && S::v_poff(j, u) == T.v_poff[j][u] &&
           S::v_soft(j, u) == T.v_soft[j][u] && S::v_mod(j, u) == T.v_mod[j][u] && S::v_first(j, u) == T.v_first[j][u] &&
           S::v_val(j, u) == T.v_val[j][u];
  ok = ok && S::off_r_body() == M.off_r_body && S::off_obst() == M.off_obst && S::off_lin() == M.off_lin &&
       S::off_wu() == M.off_wu && S::off_goal() == M.off_goal && S::off_wgoal() == M.off_wgoal &&
       S::off_wconstr() == M.off_wconstr && S::off_ws() == M.off_ws && S::has_goal() == M.has_goal &&
       S::has_avoid() == M.has_avoid;
  for (int j = 0; j < RMPC_MAX_JOINTS; j++) {
    ok = ok && S::joint_type(j) == M.joint_type[j];
    for (int c = 0; c < 3; c++)
      ok = ok && S::joint_xyz(j, c) == M.joint_xyz[j][c] && S::joint_axis(j, c) == M.joint_axis[j][c] && S::dd_off(j, c) == M.dd_off[j][c];
    for (int c = 0; c < 9; c++) ok = ok && S::joint_rot(j, c) == M.joint_rot[j][c];
  }
  return ok;
}

#if defined(RMPC_STAMPS) || defined(RMPC_RIC_STAMPS)
// reads and clears a stamp array of this unit: STAMPS_SWEEP g_sst, STAMPS_RIC g_rst (1: failed, or the build has none)
int read_stamps(const int which, long long *out) {
  const void *sym = nullptr;
#ifdef RMPC_STAMPS
  if (which == STAMPS_SWEEP) sym = &g_sst;
#endif
#ifdef RMPC_RIC_STAMPS
  if (which == STAMPS_RIC) sym = &g_rst;
#endif
  const long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!sym || hipMemcpyFromSymbol(out, sym, sizeof(z)) != hipSuccess) return 1;
  return hipMemcpyToSymbol(sym, z, sizeof(z)) != hipSuccess;
}
#endif

template <class C, class V>
VariantOps ops(const char *spec, bool (*matches)(const rmpc_desc &, const DevModel &, const DevTables &)) {
  VariantOps v{};
  v.robot = C::ROBOT; v.nq = C::NQ; v.ns = C::NS;
  v.spec = spec; v.matches = matches;
  v.fused = C::FUSED_OK || C::ARM_FUSED;
  v.arm_fused = C::ARM_FUSED;
  v.rs = C::RS;
  v.pass = launch_pass<C, V>;
  v.pass_step_debug = launch_pass_step_debug<C, V>;
  if constexpr (C::FUSED_OK) {
    v.difficulty = launch_difficulty<C>;
    v.fused_launch = launch_fused<C, V>;
    v.fused_step_debug = launch_fused_step_debug<C, V>;
  } else if constexpr (C::ARM_FUSED) {
    v.fused_launch = launch_fused_arm<C>;
    v.fused_step_debug = launch_fused_arm_step_debug<C>;
  }
  v.advance = launch_advance<C>;
  v.retarget = launch_retarget<C>;
#if defined(RMPC_STAMPS) || defined(RMPC_RIC_STAMPS)
  v.read_stamps = read_stamps;
#endif
  return v;
}

// The entries of variant C: its runtime-table view, then the generated views of its robot and size.
template <class C, bool BUILD>
bool add_variant() {
  if constexpr (BUILD) {
    constexpr RecLayout L = rec_layout(C::ROBOT, C::NQ, C::NV, C::NS, C::NX);
    static_assert(L.q == C::R_Q && L.c == C::R_C && L.dg == C::R_DG && L.cs == C::R_CS && L.q0 == C::R_Q0 && L.q1 == C::R_Q1 &&
                  L.rc == C::R_RC && L.a5 == C::R_A5 && L.b5 == C::R_B5 && L.d == C::R_D && L.rw == C::RW && L.rs == C::RS,
                  "rec_layout out of step with Cfg::R_*");
    add_variant_ops(ops<C, RtView>("", nullptr));
#define RMPC_S(ID, S, ROBOT_, NQ_, NS_) \
    if constexpr (ROBOT_ == C::ROBOT && NQ_ == C::NQ && NS_ == C::NS) add_variant_ops(ops<C, S>(#S, spec_matches<S>));
    RMPC_SPECS(RMPC_S)
#undef RMPC_S
  }
  return BUILD;
}

#define RMPC_ADD(ID, R, NQ, NS) const bool added_##ID = add_variant<Cfg<R, NQ, NS>, ((RMPC_UNIT_VARIANTS >> ID) & 1) != 0>();
RMPC_VARIANTS(RMPC_ADD)
#undef RMPC_ADD

}  // namespace
