// rmpc_loop.hpp -- the closed loop on the device, per variant: k_advance (plant step and shifted warm start), k_retarget
// (scene packing) and k_difficulty (queue order of the fused kernels).  Part of rmpc_kernels.hip (included there last,
// inside namespace rmpc); needs rmpc_solver.hpp.

// ===========================================================================
// Scene packing and closed-loop advance: device
// counterparts of the planner's host loops, so that neither the N*npar
// parameter vectors nor the plans have to cross PCIe between control steps.
// ===========================================================================
// Closed loop between two solves: the plant is the model's own ERK2 map applied to the first
// control of the previous plan, the warm start is the shifted plan (shiftHorizon,
// mpcPlanner.py:215-226) or the current state repeated (setX0 "current_state", :228-232).
constexpr int kAdvanceIB = 16;   // instances per block of k_advance
template <class C>
__global__ __launch_bounds__(256) void k_advance(const DevModel M, const double *__restrict__ zprev, double *__restrict__ xinit,
                                                 double *__restrict__ x0, int B, int previous_plan_all,
                                                 const int *__restrict__ exitflag) {
  // A block takes kAdvanceIB instances: one lane each for the plant step, then all 256 lanes shift the plans
  // element by element (contiguous in the ABI layout [b][k][j]: coalesced; one lane per instance walking its
  // N x nvar plan took 76 us for 1024 arms).
  constexpr int NX = C::NX, NS = C::NS, NV = C::NV, IB = kAdvanceIB;
  __shared__ double sx[IB][NX];
  __shared__ int spp[IB];
  const int b0 = blockIdx.x * IB, t = threadIdx.x;
  const int N = M.N;
  if (t < IB && b0 + t < B) {
    const int b = b0 + t;
    double z[NV], xn[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) z[j] = xinit[(size_t)b * NX + j];
#pragma unroll
    for (int j = NX; j < NV; j++) z[j] = zprev[(size_t)b * N * NV + j];  // slack and first control of the plan
    if constexpr (C::ROBOT == RMPC_ROBOT_CHAIN) {
      chain_step<C>(M.dt, z, xn);
    } else {
      double A5[25], B5[10];
      diffdrive_step<C>(M.dt, z, xn, A5, B5, false);
    }
#pragma unroll
    for (int j = 0; j < NX; j++) { xinit[(size_t)b * NX + j] = xn[j]; sx[t][j] = xn[j]; }
    // an instance whose last solve failed (exitflag < 0) has no plan worth shifting: it restarts from its state,
    // as the boxer example of the reference does for its linearisation point (boxer_example.py:194-198)
    spp[t] = (previous_plan_all && !(exitflag && exitflag[b] < 0)) ? 1 : 0;
  }
  __syncthreads();
  const int nb = (B - b0) < IB ? (B - b0) : IB;
  const int per = N * NV;
  for (int e = t; e < nb * per; e += 256) {
    const int ib = e / per, r = e - ib * per, k = r / NV, j = r - k * NV;
    const size_t base = (size_t)(b0 + ib) * per;
    double val;
    if (spp[ib]) val = zprev[base + (size_t)(k + 1 < N ? k + 1 : N - 1) * NV + j];
    else val = j < NX ? sx[ib][j] : 0.0;
    x0[base + r] = val;
  }
  (void)NS;
}

// Steady closed loop (the examples hand the planner a new goal whenever the driver has one,
// setGoalReaching every control step in examples/boxer_example_global.py:203-212): one lane per instance looks at the
// state the plant step has just produced and gives the instance its next goal from its pool when the end link has
// arrived (within tol of the goal) or has dwelt max_dwell control steps on this goal; an instance whose solve FAILED
// (exitflag < 0: infeasible or diverged, a state no plan leads out of) is put back to its start state with a cold
// plan and takes its next goal too.  The goals live in the scene's goal array, so the next parameter packing sees them.
struct RetargetDev {   // rmpc_retarget, device side
  double *xinit, *x0, *goal;
  const int *exitflag, *iters;
  const double *pool, *x_start, *lower, *upper;
  int P;
  int *cursor, *dwell, *failrun;
  double tol, settle_vel;
  int settle_min_dwell, max_dwell, fail_reset_after;
  long long *counts;
  double *wmu;
  double wmu_regoal;
};
template <class C>
__global__ __launch_bounds__(256) void k_retarget(const DevModel M, const DevTables *__restrict__ Tp, int B, const RetargetDev R) {
  constexpr int NQ = C::NQ, NX = C::NX, NV = C::NV;
  const int b = blockIdx.x * 256 + threadIdx.x;
  const bool in = b < B;
  long long *const counts = R.counts;
  // statistics of the control step, summed on the device (no host read inside the loop): exit flags and iterations
  if (counts && R.exitflag) {
    const int ef = in ? R.exitflag[b] : -1000;
    const int it = (in && R.iters) ? R.iters[b] : 0;
    const int cls[4] = {ef == 1, ef == 2, ef == 0, ef < 0 && ef > -1000};
    for (int c = 0; c < 4; c++) {
      const unsigned long long mk = __ballot(cls[c]);
      if ((threadIdx.x & 63) == 0 && mk) atomicAdd((unsigned long long *)&counts[4 + c], (unsigned long long)__popcll(mk));
    }
    int si = it;
    for (int off = 32; off >= 1; off >>= 1) si += __shfl_xor(si, off, 64);
    if ((threadIdx.x & 63) == 0 && si) atomicAdd((unsigned long long *)&counts[8], (unsigned long long)si);
  }
  if (!in) return;
  const RtView v(M, *Tp);
  double *const xi = R.xinit + (size_t)b * NX;
  const bool failed = R.exitflag && R.exitflag[b] < 0;
  // A failed solve (infeasible, diverged, line search): the reference prints the flag and drives on with the action it
  // got (mpcPlanner.py:263-264), its boxer example takes the current pose as the next linearisation point
  // (boxer_example.py:194-198) -- the plant step has applied the returned control, the next solve starts cold from the
  // new state (rmpc_advance_device_flags).  Only an instance that has failed fail_reset_after control steps IN A ROW is
  // put back to its start state (a reset; 0: never).
  int fr = R.failrun ? R.failrun[b] : 0;
  fr = failed ? fr + 1 : 0;
  // ... or one whose configuration has left the joint-limit box by more than a limit row's reach (a robot outside its
  // workspace: the examples' simulator stops a joint at its limit, the plant here is the bare integrator -- a short
  // horizon without a terminal set does overshoot a far goal; counted on its own, counts[12])
  bool oob = false;
  if (R.lower && R.upper) {
    for (int j = 0; j < M.n; j++) {
      const double lo = R.lower[(size_t)b * M.n + j], hi = R.upper[(size_t)b * M.n + j];
      const double margin = 0.05 * (hi - lo);
      oob |= (xi[j] < lo - margin) | (xi[j] > hi + margin);
    }
  }
  const bool reset = oob || (failed && R.fail_reset_after > 0 && fr >= R.fail_reset_after);
  if (counts && oob) atomicAdd((unsigned long long *)&counts[12], 1ull);
  if (reset) {
    for (int j = 0; j < NX; j++) xi[j] = R.x_start[(size_t)b * NX + j];
    for (int k = 0; k < M.N; k++)
      for (int j = 0; j < NV; j++) R.x0[((size_t)b * M.N + k) * NV + j] = j < NX ? R.x_start[(size_t)b * NX + j] : 0.0;
    fr = 0;
  }
  if (R.failrun) R.failrun[b] = fr;
  if (counts && fr > 0) atomicAdd((unsigned long long *)&counts[11], 1ull);
  double q[NQ];
#pragma unroll
  for (int j = 0; j < NQ; j++) q[j] = xi[j];
  Kin<C> kin;
  kin.compute(v, q);
  Vec3 J[NQ];
  const Vec3 pt = kin.template point<0>(v, J);   // slot 0: the goal's end frame (build_tables)
  double *const g = R.goal + (size_t)b * 3;
  const double dx = pt.x - g[0], dy = pt.y - g[1], dz = pt.z - g[2];
  const double dist = sqrt(dx * dx + dy * dy + dz * dz);
  const bool arrived = dist < R.tol;
  // settled: the robot has come to rest on this goal -- with the reference's objective (N w / h on the first row of a
  // module, constraint_avoidance.py:22-31) a goal next to an obstacle is an equilibrium at a distance, not a point reached
  double vmax = 0.0;
  if constexpr (C::ROBOT == RMPC_ROBOT_CHAIN) {
#pragma unroll
    for (int j = 0; j < NQ; j++) vmax = fmax(vmax, fabs(xi[NQ + j]));
  } else {
    vmax = fmax(fabs(xi[6]), fabs(xi[7]));
  }
  int dw = R.dwell[b] + 1;
  const bool settled = !arrived && R.settle_vel > 0.0 && dw >= R.settle_min_dwell && vmax < R.settle_vel;
  const bool late = R.max_dwell > 0 && dw >= R.max_dwell;
  if (arrived || settled || late || reset) {
    const int c = R.cursor[b] + 1;
    R.cursor[b] = c;
    const double *gn = R.pool + ((size_t)b * R.P + (size_t)(c % R.P)) * 3;
    g[0] = gn[0]; g[1] = gn[1]; g[2] = gn[2];
    dw = 0;
    // a new goal moves the optimum: the multipliers of the last solve stay, the barrier parameter of the next solve
    // restarts from mu_regoal (stored so that warm_mu() yields it) instead of 1000 x the converged one
    if (R.wmu && R.wmu_regoal > 0.0 && !failed) R.wmu[b] = R.wmu_regoal;
    if (counts) {
      atomicAdd((unsigned long long *)&counts[reset ? 3 : (arrived ? 0 : (settled ? 1 : 2))], 1ull);
      if (!reset) {
        atomicAdd((unsigned long long *)&counts[9], (unsigned long long)(dist * 1e6));   // distance at the hand-over [um]
        atomicAdd((unsigned long long *)&counts[10], 1ull);
      }
    }
  }
  R.dwell[b] = dw;
}

// Launch order of a COLD fused launch that is larger than the chip (more instances than half-wavefronts: the rest wait
// in the queue).  A lone launch lasts as long as its slowest instance needs from the moment it is dequeued, and the
// slow ones of a cold batch are mostly those that start close to a constraint boundary (the interior-point method's
// first steps are cut by the fraction to the boundary): on the BASELINE scenarios 37-40 of the 40 slowest of 4096
// point robots are in the closer half.  One lane per instance evaluates the distance rows (obstacle, plane, self
// collision) of the start state with the parameters of the second stage and hands k_order_t a key, closest first --
// longest-processing-time-first scheduling with an estimate instead of the previous solve's count.  What an instance
// computes does not depend on its place in the queue (test_launch_order_...).
template <class C>
__global__ __launch_bounds__(64) void k_difficulty(const DevModel M, const DevTables *__restrict__ Tp, const int B,
                                                    const double *__restrict__ xinit, const double *__restrict__ params,
                                                    int *__restrict__ key) {
  constexpr int NQ = C::NQ, NX = C::NX;
  const int b = blockIdx.x * 64 + threadIdx.x;   // (one-wavefront blocks: see k_order_t)
  if (b >= B) return;
  const RtView v(M, *Tp);
  const double *const P = params + ((size_t)b * M.N + (M.N > 1 ? 1 : 0)) * M.npar;
  double q[NQ];
#pragma unroll
  for (int j = 0; j < NQ; j++) q[j] = xinit[(size_t)b * NX + j];
  Kin<C> kin;
  kin.compute(v, q);
  const double rbody = (v.off_r_body() >= 0) ? P[v.off_r_body()] : 0.0;
  double dmin = 1e30, dseg = 1e30;
  // (slot 0 is the goal's end frame when the model has a GoalReaching objective: for its spherical obstacles also the
  //  clearance of the straight segment from the point to the goal -- an instance whose way is blocked takes longer
  //  than one that merely starts next to an obstacle; the sum of the two clearances orders the BASELINE batches
  //  almost as well as the iteration counts themselves: simulated makespans 36 / 60 / 61 / 59 / 102 / 46 iterations
  //  against 35 / 60 / 61 / 59 / 102 / 46 for the true longest-first order and 48 / 72 / 61 / 73 / 102 / 54 by index)
  const bool goal = v.has_goal() != 0;
  Vec3 gv = {0, 0, 0};
  if (goal) gv = {P[v.off_goal()], P[v.off_goal() + 1], P[v.off_goal() + 2]};
  for_range<0, kMaxSlots>([&](auto slc) __attribute__((always_inline)) {
    constexpr int SL = decltype(slc)::value;
    if (SL < v.nslots()) {
      Vec3 J[NQ];
      const Vec3 Pt = kin.template point<SL>(v, J);
      for (int r = v.slot_row_begin(SL); r < v.slot_row_begin(SL + 1); r++) {
        const int kind = v.fk_kind(r), ob = v.fk_obst(r);
        double h;
        if (kind == ROW_RADIAL) {
          const double *o = P + v.off_obst() + 4 * ob;
          const Vec3 dv = {Pt.x - o[0], Pt.y - o[1], Pt.z - o[2]};
          h = sqrt(dot(dv, dv)) - o[3] - rbody;
          if (SL == 0 && goal) {
            const Vec3 sg = {gv.x - Pt.x, gv.y - Pt.y, gv.z - Pt.z}, so = {o[0] - Pt.x, o[1] - Pt.y, o[2] - Pt.z};
            const double l2 = dot(sg, sg);
            double t = l2 > 0.0 ? dot(so, sg) / l2 : 0.0;
            t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
            const Vec3 cv = {so.x - t * sg.x, so.y - t * sg.y, so.z - t * sg.z};
            dseg = fmin(dseg, sqrt(dot(cv, cv)) - o[3] - rbody);
          }
        } else if (kind == ROW_LINEAR) {
          const double *o = P + v.off_lin() + 4 * ob;
          const Vec3 av = {o[0], o[1], o[2]};
          h = fabs(dot(av, Pt) + o[3]) / sqrt(dot(av, av)) - rbody;
        } else {
          h = sqrt(dot(Pt, Pt)) - 2.0 * rbody;
        }
        dmin = fmin(dmin, h);
      }
    }
  });
  // 256 classes of 4 cm of (clearance at the start + clearance of the way), the smallest (and every infeasible start)
  // in the class that is dequeued first
  const double dsum = (dmin > 0.0 ? dmin : 0.0) + (dseg < 1e29 ? (dseg > 0.0 ? dseg : 0.0) : (dmin > 0.0 ? dmin : 0.0));
  const double c = dsum * 25.0;
  key[b] = 255 - (c < 255.0 ? (int)c : 255);
}
