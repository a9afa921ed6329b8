// rmpc_inst.hpp -- the per-instance decision logic: the solver words of an instance (Inst), the whole-horizon
// reductions (wave_*, Reduced), inst_decide and inst_after_recursion.  Part of rmpc_kernels.hip (included there, inside
// namespace rmpc); the pass kernels and both fused kernels run this one copy.  Needs rmpc_solver.hpp.

// reductions over the LPI consecutive lanes that work on one instance (a whole wavefront or half of one)
//
// The value of the partner lane of a butterfly level OFF.  XCHG_SHFL: __shfl_xor, lane ^ OFF through the LDS crossbar
// (ds_bpermute_b32 per word and a wait for its answer: a dependent LDS round trip per level, on the CU's LDS queue behind
// the other wavefronts).  XCHG_DPP: vector moves inside the SIMD, no LDS instruction and no counter to wait for --
//   32, 16  v_permlane32_swap_b32 / v_permlane16_swap_b32 (gfx950) of the word with a copy of itself: the instruction swaps
//           the odd halves / odd 16-lane rows of its first operand with the even ones of its second, so the partner's
//           word is in the first operand for a lane of an odd half / row and in the second for the others (one select
//           per word): exactly lane ^ 32 / lane ^ 16;
//   8       row_ror:8, exactly lane ^ 8 (a rotation by half a row);
//   4       row_ror:4, the lane four places round its row: lane ^ 4 or (lane ^ 4) ^ 8;
//   2, 1    quad_perm [2, 3, 0, 1] / [1, 0, 3, 2], exactly lane ^ 2 / lane ^ 1.
// Same results as the shuffle tree bit for bit, level by level in the same order (LPI / 2 .. 1) with the lane's own
// value as the first operand: every level but 4 reads lane ^ OFF itself; at level 4 the lane read is either lane ^ 4 or
// its level-8 partner, and after the level-8 step a lane and its level-8 partner hold the same word -- a + b and b + a,
// or max / min of the same pair, and the hardware's add, max and min are commutative down to the bits: the sum of +0
// and -0 is +0 either way, v_max_f64 / v_min_f64 order -0 below +0 whichever operand holds it, and return the other
// operand when one is a NaN.  NaNs are the one exception: with two NaNs the payload returned may depend on the operand
// order, so a result that is NaN is NaN in the same lanes as with the shuffle tree, with a payload that is not pinned
// (nothing reads payloads; the kernel's max operands are absolute values and products of positive numbers).
// tests/test_gpu_wave_reduce.py compares the two forms lane by lane (rmpc_debug_wave_reduce).
//
// A DPP or permlane move reads a register of another lane, and that lane must be active: XCHG_DPP needs all LPI lanes of
// the instance in the call (level 16 pairs the two rows of a half, level 32 the two halves; the other levels stay inside
// a 16-lane row).  Every call site has them -- whole wavefronts, or whole halves where LPI = 32 and a half can sit the
// call out (noted at each) --; one that could be entered by a part of an instance's lanes has to ask for XCHG_SHFL.
// (arm_sweep_call asks for it for another reason, given there.)
constexpr bool XCHG_DPP = true, XCHG_SHFL = false;
template <int OFF, bool DPP>
__device__ __forceinline__ double lane_xchg(const double v) {
  static_assert(OFF == 32 || OFF == 16 || OFF == 8 || OFF == 4 || OFF == 2 || OFF == 1, "lane_xchg: a butterfly level of a wavefront");
  if constexpr (!DPP) return __shfl_xor(v, OFF, 64);
  else if constexpr (OFF >= 16) {
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const bool odd = (threadIdx.x & OFF) != 0;   // (blocks are whole wavefronts: bit OFF of the lane index)
    if constexpr (OFF == 32) {
      const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
      return __hiloint2double((int)(odd ? b[0] : b[1]), (int)(odd ? a[0] : a[1]));
    } else {
      const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
      return __hiloint2double((int)(odd ? b[0] : b[1]), (int)(odd ? a[0] : a[1]));
    }
  }
  else if constexpr (OFF == 8) return dpp_move<0x128>(v);   // row_ror:8
  else if constexpr (OFF == 4) return dpp_move<0x124>(v);   // row_ror:4
  else if constexpr (OFF == 2) return dpp_move<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  else return dpp_move<0xB1>(v);                            // quad_perm [1, 0, 3, 2]
}
// fn(integral_constant<int, OFF>) for the levels OFF = LPI / 2 .. 1 of the butterfly, in that order
template <int LPI, class F>
__device__ __forceinline__ void wave_levels(F &&fn) {
  static_assert(LPI == 32 || LPI == 64, "wave_levels: a whole wavefront or half of one");
  if constexpr (LPI == 64) fn(std::integral_constant<int, 32>{});
  fn(std::integral_constant<int, 16>{});
  fn(std::integral_constant<int, 8>{});
  fn(std::integral_constant<int, 4>{});
  fn(std::integral_constant<int, 2>{});
  fn(std::integral_constant<int, 1>{});
}
template <int LPI, bool DPP = XCHG_DPP>
__device__ __forceinline__ double wave_sum(double v) {
  wave_levels<LPI>([&](auto off) __attribute__((always_inline)) { v += lane_xchg<decltype(off)::value, DPP>(v); });
  return v;
}
template <int LPI, bool DPP = XCHG_DPP>
__device__ __forceinline__ double wave_max(double v) {
  wave_levels<LPI>([&](auto off) __attribute__((always_inline)) { v = fmax(v, lane_xchg<decltype(off)::value, DPP>(v)); });
  return v;
}
template <int LPI, bool DPP = XCHG_DPP>
__device__ __forceinline__ double wave_min(double v) {
  wave_levels<LPI>([&](auto off) __attribute__((always_inline)) { v = fmin(v, lane_xchg<decltype(off)::value, DPP>(v)); });
  return v;
}

// Several reductions at once, step by step: the exchanges of one step of all of them are issued together (with the
// shuffle form a single reduction is a chain of dependent LDS-crossbar round trips; done one after the other, eleven of
// them cost eleven chains; with the vector moves a step pays the wait states between an operand's last write and the
// move that reads it once, not once per value).  Same partner pattern, hence the same rounding, as wave_sum / wave_max /
// wave_min.
template <int LPI, bool DPP = XCHG_DPP, int NS_, int NM_, int NN_>
__device__ __forceinline__ void wave_reduce_many(double (&sums)[NS_], double (&maxs)[NM_], double (&mins)[NN_]) {
  wave_levels<LPI>([&](auto off) __attribute__((always_inline)) {
    constexpr int OFF = decltype(off)::value;
    double ts[NS_], tm[NM_], tn[NN_];
#pragma unroll
    for (int i = 0; i < NS_; i++) ts[i] = lane_xchg<OFF, DPP>(sums[i]);
#pragma unroll
    for (int i = 0; i < NM_; i++) tm[i] = lane_xchg<OFF, DPP>(maxs[i]);
#pragma unroll
    for (int i = 0; i < NN_; i++) tn[i] = lane_xchg<OFF, DPP>(mins[i]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NS_; i++) sums[i] += ts[i];
#pragma unroll
    for (int i = 0; i < NM_; i++) maxs[i] = fmax(maxs[i], tm[i]);
#pragma unroll
    for (int i = 0; i < NN_; i++) mins[i] = fmin(mins[i], tn[i]);
  });
}

// ---- per-instance solver state ------------------------------------------------------------------------
// One set of words per instance.  The pass kernels keep them in the workspace (arrays over the batch), the
// fused kernel in registers of the wavefront that owns the instance; the decision logic is the same code.
struct Inst {
  double mu, rho, phi0, Dd, fcur, thcur, logcur, res_stat, res_eq, res_ineq, res_comp, obj;
  double amin_p, amin_d;   // fraction-to-the-boundary step lengths of the current step
  double mu_hold;          // barrier restart: the level mu is held at (0: none)
  int status, iters, ls, ls0, lsst, cur, newstep, redo, force_gn, gn_sticky, curv_fail, usedc, stall, curv_skip, curv_back;
  int small_steps;         // barrier restart: accepted short steps in a row
  double theta_mem, theta_c;      // scaled curvature: the scale the next curvature step starts from / of this iteration
  int theta_clean, theta_retry;   // accepted curvature steps in a row without a retry / this iteration has retried
};
__device__ __forceinline__ void inst_init(Inst &s, double mu0) {
  s.mu = mu0; s.rho = 0.0; s.phi0 = 0.0; s.Dd = 0.0; s.fcur = 0.0; s.thcur = 0.0; s.logcur = 0.0;
  s.res_stat = 0.0; s.res_eq = 0.0; s.res_ineq = 0.0; s.res_comp = 0.0; s.obj = 0.0;
  s.amin_p = 1.0; s.amin_d = 1.0;
  s.status = ST_ACTIVE; s.iters = 0; s.ls = 0; s.ls0 = 0; s.lsst = 0; s.cur = 0; s.newstep = 0; s.redo = 0;
  s.force_gn = 0; s.gn_sticky = 0; s.curv_fail = 0; s.usedc = 0; s.stall = 0; s.curv_skip = 0; s.curv_back = 0;
  s.small_steps = 0; s.mu_hold = 0.0;
  s.theta_mem = 1.0; s.theta_c = 1.0; s.theta_clean = 0; s.theta_retry = 0;
}
__device__ __forceinline__ void inst_load(Inst &s, const Ws &W, int b) {
  s.mu = W.mu[b]; s.rho = W.rho[b]; s.phi0 = W.phi0[b]; s.Dd = W.Dd[b]; s.fcur = W.fcur[b]; s.thcur = W.thcur[b];
  s.logcur = W.logcur[b]; s.res_stat = W.res_stat[b]; s.res_eq = W.res_eq[b]; s.res_ineq = W.res_ineq[b];
  s.res_comp = W.res_comp[b]; s.obj = W.obj[b];
  s.amin_p = __longlong_as_double((long long)W.amin_p[b]); s.amin_d = __longlong_as_double((long long)W.amin_d[b]);
  s.status = W.status[b]; s.iters = W.iters[b]; s.ls = W.ls[b]; s.ls0 = W.ls0[b]; s.lsst = W.lsst[b]; s.cur = W.cur[b];
  s.newstep = W.newstep[b]; s.redo = W.redo[b]; s.force_gn = W.force_gn[b]; s.gn_sticky = W.gn_sticky[b];
  s.curv_fail = W.curv_fail[b]; s.usedc = W.usedc[b]; s.stall = W.stall[b]; s.curv_skip = W.curv_skip[b]; s.curv_back = W.curv_back[b];
  s.small_steps = W.small_steps[b]; s.mu_hold = W.mu_hold[b];
  s.theta_mem = W.theta_mem[b]; s.theta_c = W.theta_c[b]; s.theta_clean = W.theta_clean[b]; s.theta_retry = W.theta_retry[b];
}
__device__ __forceinline__ void inst_store(const Inst &s, const Ws &W, int b) {
  W.mu[b] = s.mu; W.rho[b] = s.rho; W.phi0[b] = s.phi0; W.Dd[b] = s.Dd; W.fcur[b] = s.fcur; W.thcur[b] = s.thcur;
  W.logcur[b] = s.logcur; W.res_stat[b] = s.res_stat; W.res_eq[b] = s.res_eq; W.res_ineq[b] = s.res_ineq;
  W.res_comp[b] = s.res_comp; W.obj[b] = s.obj;
  W.amin_p[b] = (unsigned long long)__double_as_longlong(s.amin_p); W.amin_d[b] = (unsigned long long)__double_as_longlong(s.amin_d);
  W.status[b] = s.status; W.iters[b] = s.iters; W.ls[b] = s.ls; W.ls0[b] = s.ls0; W.lsst[b] = s.lsst; W.cur[b] = s.cur;
  W.newstep[b] = s.newstep; W.redo[b] = s.redo; W.force_gn[b] = s.force_gn; W.gn_sticky[b] = s.gn_sticky;
  W.curv_fail[b] = s.curv_fail; W.usedc[b] = s.usedc; W.stall[b] = s.stall; W.curv_skip[b] = s.curv_skip; W.curv_back[b] = s.curv_back;
  W.small_steps[b] = s.small_steps; W.mu_hold[b] = s.mu_hold;
  W.theta_mem[b] = s.theta_mem; W.theta_c[b] = s.theta_c; W.theta_clean[b] = s.theta_clean; W.theta_retry[b] = s.theta_retry;
}

// whole-horizon sums / maxima of the trial point the last sweep evaluated (+ the merit slope of the step)
struct Reduced { double f, th, lgs, rstat, req, rineq, rcomp, sumc, minc, badf, gphi; };
// one stage's partials of instance b, as k_sweep / k_step left them in the workspace, into r (the pass kernels' stage loops)
__device__ __forceinline__ void reduced_add(Reduced &r, const Ws &W, const int k, const int b, const bool first) {
  r.f += W.part[IDX(P_F, k, b)];
  r.th += W.part[IDX(P_TH, k, b)];
  r.lgs += W.part[IDX(P_LOGS, k, b)];
  r.rstat = fmax(r.rstat, W.part[IDX(P_RSTAT, k, b)]);
  r.req = fmax(r.req, W.part[IDX(P_REQ, k, b)]);
  r.rineq = fmax(r.rineq, W.part[IDX(P_RINEQ, k, b)]);
  r.rcomp = fmax(r.rcomp, W.part[IDX(P_RCOMP, k, b)]);
  r.sumc += W.part[IDX(P_SUMC, k, b)];
  r.minc = fmin(r.minc, W.part[IDX(P_MINC, k, b)]);
  r.badf += W.part[IDX(P_BAD, k, b)];
  r.gphi += first ? 0.0 : W.gphi[(size_t)k * W.Bp + b];
}

// Armijo test of the trial point, acceptance, barrier update, convergence tests.  Returns true when a new
// step has to be computed (Riccati recursion next; `usec`: with the exact constraint curvature); false when
// the instance retries with a shorter step, re-evaluates (null pass) or has stopped (s.status).
template <class C>
__device__ __forceinline__ bool inst_decide(const DevModel &M, Inst &s, const Reduced &r, const bool first, bool &usec) {
  const int N = M.N;
  s.newstep = 0;
  double mu = s.mu;
  int status = ST_ACTIVE;
  int iters = s.iters;
  const bool redo = (!first) && (s.redo != 0);
  int lsst = first ? 0 : s.lsst;
  double alpha_acc = 1.0;   // length of the step accepted in this pass (barrier restart)
  usec = false;
  if (first) {
    if (r.badf != 0.0) status = -7;  // inverse-barrier row not strictly feasible at the start
  } else if (redo) {
    // null pass: same point, the step is recomputed below with the Gauss-Newton blocks
    s.redo = 0;
  } else {
    const double a0 = s.amin_p;
    int ls = s.ls;
    double rho = s.rho, phi0 = s.phi0, Dd = s.Dd;
    if (ls == s.ls0) {   // first trial of this line search
      const double thc = s.thcur;
      if (thc > 1e-13) {
        const double need = r.gphi / (0.9 * thc);
        if (rho < need) rho = need + 1.0;
      }
      Dd = r.gphi - rho * thc;
      phi0 = s.fcur - mu * s.logcur + rho * thc;
      s.rho = rho; s.phi0 = phi0; s.Dd = Dd;
    }
    const double alpha = ldexp(a0, -ls);
    const double phi = r.f - mu * r.lgs + rho * r.th;
    const bool ok = (r.badf == 0.0) && (phi <= phi0 + kArmijo * alpha * Dd + 1e-13 * fabs(phi0));
    const int usedc = s.usedc;
    if (!ok) {
      ls++;
      if (ls > (usedc ? kLsCurv - 1 : M.ls_max)) {
        if (usedc) {
          // the curvature step failed its line search: recompute this iteration's step with
          // the Gauss-Newton blocks (null pass next); latch after repeated failures
          if constexpr (C::BACKOFF) {
            // (the unicycle, the small chains: the next curvature steps are skipped -- 1, 2, 4 .. 16 iterations, doubling
            //  with every failure in a row, over after a success -- instead of a latch: DESIGN.md 3)
            s.curv_back = s.curv_back ? (s.curv_back < kCurvBackMax ? 2 * s.curv_back : kCurvBackMax) : 1;
            s.curv_skip = s.curv_back;
          } else {
            const int cf = s.curv_fail + 1;
            s.curv_fail = cf;
            if (cf >= kCurvFailMax) s.gn_sticky = 1;
          }
          s.redo = 1;
          s.force_gn = 1;
          s.ls = 0;
          return false;
        }
        s.status = -8;  // line search failure; the current iterate is returned
        return false;
      }
      s.ls = ls;
      return false;  // next sweep retries with alpha / 2
    }
    if (usedc) { s.curv_fail = 0; s.curv_back = 0; }
    if constexpr (C::CSCALE) {
      // scaled curvature: the scale that needed a retry is kept, kCsClean accepted curvature steps in a row without a
      // retry double it again; an iteration whose retries all failed (Gauss-Newton step accepted) keeps the last scale
      if (usedc) {
        if (s.theta_retry) { s.theta_mem = s.theta_c; s.theta_clean = 0; }
        else if (++s.theta_clean >= kCsClean) { s.theta_mem = s.theta_c < 0.75 ? 2.0 * s.theta_c : 1.0; s.theta_clean = 0; }
      } else if (s.theta_retry) { s.theta_mem = s.theta_c; s.theta_clean = 0; }
    }
    // the arms: a Gauss-Newton step accepted at full length releases the latch (the failures that set it belong to
    // the first iterations of a warm start, where the fraction to the boundary cuts the steps)
    if constexpr (C::FKCURV) {
      if (!usedc && ls == 0) { s.gn_sticky = 0; s.curv_fail = 0; }
    }
    // step-length memory: the next Gauss-Newton line search starts one halving above the accepted one (models
    // whose steps overshoot every iteration -- the unicycle -- otherwise pay a pass per halving per iteration)
    lsst = ls > kLsGrow ? ls - kLsGrow : 0;
    s.lsst = lsst;
    alpha_acc = alpha;
    iters++;
  }
  // ---- accept the trial point ------------------------------------------------------
  if (status == ST_ACTIVE) {
    const double f_prev = s.fcur;
    const int stall0 = s.stall;
    s.cur ^= 1;
    s.fcur = r.f;
    s.thcur = r.th;
    s.logcur = r.lgs;
    if (!redo) {
      s.iters = iters;
      s.res_stat = r.rstat; s.res_eq = r.req; s.res_ineq = r.rineq; s.res_comp = r.rcomp; s.obj = r.f;
      if (!first) {
        // LOQO-style centrality rule with floors (DESIGN.md, section "Algorithm")
        const double cnt = (double)N * (double)M.m;
        const double avg = r.sumc / cnt;
        const double xi = r.minc / avg;
        double sg = 0.05 * (1.0 - xi) / xi;
        if (sg > 2.0) sg = 2.0;
        sg = 0.1 * sg * sg * sg;
        if (sg < 0.02) sg = 0.02;
        if (sg > 0.8) sg = 0.8;
        mu = sg * avg;
        if (mu < 0.1 * M.tol_comp) mu = 0.1 * M.tol_comp;
        // barrier restart on stalled steps (oracle: ORC_RS_*): from iteration kRsIt on, kRsN accepted steps in
        // a row shorter than kRsAlpha while mu < kRsMu -- the iterate crawls along a boundary with the barrier at its
        // floor -- hold mu at kRsMu, released by the factor kRsDecay per iteration
        {
          int ss = (iters - 1 >= kRsIt && alpha_acc < kRsAlpha) ? s.small_steps + 1 : 0;
          double mh = s.mu_hold;
          if (ss >= kRsN && mu < kRsMu && !(mh > 0.0)) { mh = kRsMu; ss = 0; }
          if (mh > 0.0) {
            if (mu < mh) mu = mh;
            mh *= kRsDecay;
            if (mh < 0.1 * M.tol_comp) mh = 0.0;
          }
          s.small_steps = ss; s.mu_hold = mh;
        }
        s.mu = mu;
        if (!(mu < kMuDiverged)) status = -7;
      }
      if (status == ST_ACTIVE) {
        if (!isfinite(r.rstat) || !isfinite(r.req) || !isfinite(r.rineq)) status = -6;
        else if (r.rstat <= M.tol_stat && r.req <= M.tol_eq && r.rineq <= M.tol_ineq && r.rcomp <= kCompFrac * M.tol_comp) status = 1;
        else {
          // acceptable termination: feasible, complementary, objective stagnant for acc_iters iterations
          int stall = stall0;
          if (!first && r.req <= kAccFeas && r.rineq <= kAccFeas && r.rcomp <= kAccFeas &&
              fabs(r.f - f_prev) <= M.acc_obj_tol * fmax(1.0, fabs(r.f)))
            stall++;
          else
            stall = 0;
          s.stall = stall;
          if (M.acc_iters > 0 && stall >= M.acc_iters) status = 2;
          else if (iters >= M.max_iter) status = 0;
        }
      }
    }
  }
  if (status != ST_ACTIVE) {
    s.status = status;
    return false;
  }
  // exact constraint curvature unless latched off or this is the fallback pass
  if constexpr (C::CURV || C::DDCURV) usec = M.use_curv && !s.gn_sticky && !s.force_gn && (mu <= kCurvMu);
  if constexpr (C::BACKOFF) {
    // (a fallback pass -- force_gn -- is not an iteration of its own: the skip counter moves once per iteration)
    if (usec && s.curv_skip > 0) { s.curv_skip--; usec = false; }
  }
  s.force_gn = 0;
  if constexpr (C::CSCALE) {
    if (!redo) { s.theta_c = s.theta_mem; s.theta_retry = 0; }   // (a null pass belongs to the iteration that asked for it)
  }
  // a step with the exact curvature is tried at full length first
  const int lsb = usec ? 0 : lsst;
  s.ls = lsb;
  s.ls0 = lsb;
  return true;
}
// after the recursion: a failed factorisation either falls back to Gauss-Newton (null pass) or stops the instance
__device__ __forceinline__ void inst_after_recursion(Inst &s, const bool chol_ok, const bool usec, const bool backoff = false,
                                                     const bool cscale = false) {
  if (!chol_ok) {
    if (usec) {
      if (cscale && s.theta_c > kCsMin) {
        // scaled curvature: the same iteration again (null pass next) with the curvature terms at half their weight
        s.theta_c *= 0.5; s.theta_retry = 1; s.redo = 1; s.usedc = 0;
        return;
      }
      if (backoff) {   // (diff-drive: see inst_decide)
        s.curv_back = s.curv_back ? (s.curv_back < kCurvBackMax ? 2 * s.curv_back : kCurvBackMax) : 1;
        s.curv_skip = s.curv_back;
      }
      // reduced Hessian not positive definite with the curvature terms: recompute this
      // iteration's step with the Gauss-Newton blocks (null pass next); not counted as a
      // line-search failure
      s.redo = 1; s.force_gn = 1; s.usedc = 0;
      return;
    }
    s.status = -5;
    return;
  }
  s.usedc = usec ? 1 : 0;
  s.newstep = 1;
  s.amin_p = 1.0;   // the step kernel takes the minima next
  s.amin_d = 1.0;
}
// The same on the stored words of instance b, for the pass kernels: they keep no Inst across the recursion, only the two
// words the rule reads (theta_c, curv_back, as inst_decide left them).  The rule runs on a local Inst whose other words
// start at a value it never assigns, and every word it assigned goes to the workspace: what inst_load, the rule and
// inst_store would leave there (tests/host/after_recursion_check.cpp compares the two over all cases).
template <class C>
__device__ __forceinline__ void store_after_recursion(const Ws &W, const int b, const bool chol_ok, const bool usec,
                                                      const double theta_c, const int curv_back) {
  Inst s;
  s.theta_c = theta_c; s.curv_back = curv_back;
  s.theta_retry = -1; s.redo = -1; s.force_gn = -1; s.usedc = -1; s.curv_skip = -1; s.newstep = -1;
  s.status = ST_ACTIVE; s.amin_p = 0.0; s.amin_d = 0.0;
  inst_after_recursion(s, chol_ok, usec, C::BACKOFF, C::CSCALE);
  if (s.theta_retry >= 0) { W.theta_c[b] = s.theta_c; W.theta_retry[b] = s.theta_retry; }
  if (s.redo >= 0) W.redo[b] = s.redo;
  if (s.force_gn >= 0) W.force_gn[b] = s.force_gn;
  if (s.usedc >= 0) W.usedc[b] = s.usedc;
  if (s.curv_skip >= 0) { W.curv_back[b] = s.curv_back; W.curv_skip[b] = s.curv_skip; }
  if (s.status != ST_ACTIVE) W.status[b] = s.status;
  if (s.newstep >= 0) W.newstep[b] = s.newstep;
  if (s.amin_p != 0.0) W.amin_p[b] = (unsigned long long)__double_as_longlong(s.amin_p);   // (k_step takes the minima next)
  if (s.amin_d != 0.0) W.amin_d[b] = (unsigned long long)__double_as_longlong(s.amin_d);
}
