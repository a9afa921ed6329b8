// rmpc_kernels.hip -- batched multiple-shooting interior-point MPC solver for
// MI355X (gfx950).  Replaces the FORCES Pro generated solver behind
// robotmpcs.planner.mpcPlanner.MPCPlanner.solve() (mpcPlanner.py:262).
//
// One solve = pack, then passes of three kernels until every instance has
// stopped, then unpack:
//
//   k_sweep   one lane per (instance, stage): forms the trial point
//             z + alpha dz (t, lambda, nu likewise), evaluates dynamics, cost,
//             inequality rows and their Jacobians there, condenses the barrier
//             terms into the stage record (Hessian / gradient blocks) and writes
//             the merit and KKT partial sums of the stage.   [HBM / request bound]
//   k_riccati one wavefront per instance, stage matrices in LDS: reduces the
//             stage partials, runs the Armijo test on the l1 merit, updates the
//             barrier parameter, checks convergence and runs the block-
//             tridiagonal Riccati recursion (backward, forward, costates).
//                                    [LDS throughput / LDS round-trip latency]
//   k_step    one lane per (instance, stage): fraction-to-the-boundary partial
//             minima of the slack and multiplier steps, merit slope partials.
//                                                                  [HBM bound]
//   (+ k_compact: list of the instances still iterating; k_migrate: their move
//    to a small dense workspace once few are left)
//
// Data layout: what the stage-parallel kernels exchange is [slot][stage][instance]
// with the instance index contiguous (a wavefront's 64 lanes move 512 contiguous
// bytes per slot); what the wave-per-instance kernel reads or keeps is
// [instance][stage][record] (one request per record).  Iterates are double
// buffered per instance (cur / cur^1): a trial point is written once and
// accepted by flipping a bit.  DESIGN.md, sections 4 and 5.
//
// This file is the device code that both kinds of translation unit include:
// rmpc_variants.hip instantiates the kernel templates of some kernel variants,
// rmpc_host.hip adds the kernels that do not depend on a variant (pack, unpack,
// compaction, migration, scene packing, ...) and the host side.  The code itself
// is in one header per kernel family, included below in order of dependence.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "rmpc_model.hpp"
#include "rmpc_spec_gen.hpp"   // generated views of the shipped configurations (scripts/gen_specs.py)

namespace rmpc {

#include "rmpc_solver.hpp"         // constants, the workspace Ws, IDX, small helpers
#include "rmpc_sweep.hpp"          // sweep_body, k_sweep (+ rmpc_stamps.hpp: the stamp recorders)
#include "rmpc_inst.hpp"           // per-instance state and decisions (inst_decide, inst_after_recursion)
#include "rmpc_riccati.hpp"        // the Riccati recursion (riccati_recursion; + rmpc_ric_common.hpp: what the paths share,
                                   //  and one header per path: rmpc_ric_point / _slack / _dd / _arm / _dense.hpp)
#include "rmpc_pass_riccati.hpp"   // k_riccati, k_riccati_lane
#include "rmpc_step.hpp"           // step_body, k_step
#include "rmpc_fused.hpp"          // k_fused
#include "rmpc_arm_fused.hpp"      // the arms in one launch (k_fused_arm: a wavefront per instance, a stage per P lanes)
#include "rmpc_loop.hpp"           // k_advance, k_retarget, k_difficulty

}  // namespace rmpc
