/*
 * rmpc.h -- C ABI of the MI355X batched MPC solver (librmpc_hip.so).
 *
 * Drop-in boundary for the one native call the reference planner makes per
 * control step:
 *
 *   forcespro.nlp.Solver.from_directory(dir)            robotmpcs/planner/mpcPlanner.py:73
 *   output, exitflag, info = solver.solve(problem)      robotmpcs/planner/mpcPlanner.py:262
 *     problem = { "xinit": (nx,), "x0": (N*nvar,), "all_parameters": (N*npar,) }   :246-250
 *     output  = { "x01": (nvar,), ... }                                            :265-281
 *
 * The FORCES Pro generated solver is a per-model shared object loaded through
 * ctypes; this library is its replacement with a leading batch axis B.  Plain
 * pointers and sizes only -- no torch / numpy types cross this boundary.
 *
 * Layout at the ABI (row-major, instance-major, exactly x0.flatten() of the
 * reference, mpcPlanner.py:249):
 *   xinit  [B][nx]
 *   x0     [B][N][nvar]      nvar = nx + ns + nu, stage vector z = [x; s; u]   (mpcBase.py:76-80)
 *   params [B][N][npar]      stride npar per stage                             (mpcPlanner.py:91-104)
 *   z_out  [B][N][nvar]      row k = output["x%0*d" % (k+1)]                    (mpcPlanner.py:265-273)
 *
 * Ownership: the caller owns every in/out buffer; the library owns the handle
 * and its device workspace and keeps no caller pointer past return.
 * Threading: a handle is not thread-safe; distinct handles (one per GPU) may be
 * driven from distinct host threads or processes.
 * Errors: functions return 0 on success, non-zero on API misuse or HIP errors
 * (text via rmpc_last_error()).  Solver outcomes are per instance in exitflag:
 *    1 converged, 2 acceptable (feasible, objective stagnated -- cf. IPOPT's
 *    acceptable level), 0 iteration cap reached (plans with flag >= 0 are usable),
 *   <0 failure (-5 factorisation, -6 non-finite, -7 infeasible/diverged,
 *      -8 line search) -- the planner only tests the sign (mpcPlanner.py:263,
 *      examples/boxer_example.py:194).
 *
 * The Python binding is derived from the declarations in this file (robot_mpcs_amd/_abi.py reads the structs, the
 * prototypes and the integer macros as written here, and refuses a form it does not know: DESIGN.md 1.1).  Parameters
 * that take a device pointer are named d_*: the binding passes those, and void *, as plain addresses, and every other
 * pointer parameter as a typed host array.
 */
#ifndef RMPC_H
#define RMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 0.1.4 (104): rmpc_set_pass_budget; curvature terms of the arms.
 * 0.1.5 (105): rmpc_is_async, rmpc_retarget_device (round 3; the macro was not bumped then).
 * 0.2.0 (200): rmpc_retarget_device takes an rmpc_retarget struct (failed solves keep their state, settled robots,
 *              64-bit counters: NOT source compatible with 0.1.5), rmpc_advance_obstacles_device; rmpc_is_fused is 1
 *              for the arms with 5 .. 7 joints as well (k_fused_arm).
 * 0.2.1 (201): RMPC_MOD_ROWS -- constraint modules given as row descriptions (rmpc_desc grows by the xrow_* arrays at
 *              its end; a descriptor of the 0.2.0 size is still accepted and has no such rows).
 *              Added without a change of the macro (source and binary compatible): the global planner,
 *              RMPC_GRID_MAX_CELLS, rmpc_grid_inflate_device, rmpc_grid_fields_device, rmpc_grid_paths_device,
 *              rmpc_grid_cells_device, rmpc_follow_path_device; the lidar, rmpc_lidar, rmpc_lidar_scan_device,
 *              rmpc_plan_points_device (rmpc_free_space_device now runs on the device of d_points); fleet
 *              separation, rmpc_fleet_points_device, rmpc_fleet_planes_device; the test hook rmpc_debug_step_curv
 *              (rmpc_debug_step is that call at the weight 0 without out_C, results unchanged); the map from the
 *              scans, rmpc_grid_mark, rmpc_grid_mark_device, rmpc_grid_occupancy_device; exploration,
 *              RMPC_GRID_BAD_SEED, rmpc_grid_frontier_device, rmpc_grid_fields_seeded_device,
 *              rmpc_grid_descend_device; coordinated exploration, RMPC_ASSIGN_MAX_ROBOTS, RMPC_ASSIGN_MAX_TARGETS,
 *              rmpc_grid_targets_device, rmpc_grid_route_costs_device, rmpc_assign_greedy_device; localisation,
 *              RMPC_MATCH_MAX_RAYS, rmpc_scan_match, rmpc_grid_edge_distance_device, rmpc_lidar_project_device,
 *              rmpc_scan_match_device; moving obstacles, RMPC_TRACK_MAX_RAYS, RMPC_TRACK_MAX_TRACKS,
 *              RMPC_TRACK_MAX_DET, rmpc_tracks, rmpc_lidar_tracks_device; the fleet in the scan, rmpc_lidar_bodies,
 *              rmpc_lidar_scan_fleet_device; the test hook rmpc_last_solve_path (RMPC_PATH_*); wide-window
 *              localisation, RMPC_SEARCH_MAX_N, rmpc_scan_search, rmpc_grid_min_pyramid_device,
 *              rmpc_scan_search_work_bytes, rmpc_scan_search_device. */
#define RMPC_VERSION 201

#define RMPC_MAX_JOINTS 8
#define RMPC_MAX_LINKS 8
#define RMPC_MAX_PAIRS 4
#define RMPC_MAX_MODULES 8
#define RMPC_NV_MAX 24

/* robot kinds (base_type in the YAML, mpcBase.py:52-60) */
#define RMPC_ROBOT_CHAIN 0     /* holonomic URDF chain: nx = 2n, nu = n (mpcModel.py:65-69) */
#define RMPC_ROBOT_DIFFDRIVE 1 /* diff-drive base, fk.n() == 0 (diff_drive_mpc_model.py:24-41) */

/* inequality modules = YAML class names (models/inequalities/__init__.py) */
#define RMPC_MOD_RADIAL 0
#define RMPC_MOD_LINEAR 1
#define RMPC_MOD_SELFCOLLISION 2
#define RMPC_MOD_JOINTLIMIT 3
#define RMPC_MOD_VELLIMIT 4
#define RMPC_MOD_INPUTLIMIT 5
/* A user-defined module (a YAML constraint name that is none of the six classes above): its rows are described one by
 * one in rmpc_desc::xrow_* -- variants of the six kinds (other frames, other joints, own parameter entries) need no
 * rebuild of the library.  The reference resolves such a name to a user class by getattr
 * (robotmpcs/models/inequalities/InequalityManager.py:17-21) and lets CasADi differentiate it; here the row kinds the
 * kernels evaluate are the vocabulary. */
#define RMPC_MOD_ROWS 6
#define RMPC_MAX_XROWS 32
/* row kinds of RMPC_MOD_ROWS (value h >= 0; r_body = the model's off_r_body entry) */
#define RMPC_ROW_RADIAL 0 /* ||fk_a(q) - c|| - r - r_body, (c, r) = 4 parameters at xrow_poff (RadialConstraints.py:6-23) */
#define RMPC_ROW_LINEAR 1 /* |n . fk_a(q) + d| / ||n|| - r_body, (n, d) = 4 parameters at xrow_poff (LinearConstraints.py:8-40) */
#define RMPC_ROW_SELF 2   /* ||fk_a(q) - fk_b(q)|| - 2 r_body (SelfCollisionAvoidanceConstraints.py:8-27) */
#define RMPC_ROW_VAR 3    /* b = +1: z_a - limit, b = -1: limit - z_a, limit = the parameter at xrow_poff
                             (JointLimitConstraints.py:8-31, InputLimitConstraints.py:7-29) */

#define RMPC_JOINT_FIXED 0
#define RMPC_JOINT_REVOLUTE 1
#define RMPC_JOINT_PRISMATIC 2

/* Model descriptor: the numeric content of <solver dir>/rmpc_model.yaml, i.e.
 * what the reference encodes in the generated solver (mpcModel.py:74-126). */
typedef struct rmpc_desc {
  int32_t struct_size; /* sizeof(rmpc_desc), checked */
  int32_t device;      /* HIP device ordinal */
  int32_t robot;
  int32_t N;           /* horizon (time_horizon) */
  int32_t n, nx, nu, ns, npar;
  double dt;           /* time_step; integrator ERK2 (explicit midpoint), 5 nodes */
  int32_t n_modules;
  int32_t module_kind[RMPC_MAX_MODULES];
  int32_t nobst;       /* number_obstacles */
  int32_t n_links;
  int32_t link_frame[RMPC_MAX_LINKS];
  int32_t n_pairs;
  int32_t pair_frame[RMPC_MAX_PAIRS][2];
  int32_t end_frame;
  int32_t n_joints;
  int32_t joint_type[RMPC_MAX_JOINTS];
  int32_t joint_dof[RMPC_MAX_JOINTS];
  double joint_xyz[RMPC_MAX_JOINTS][3];
  double joint_rot[RMPC_MAX_JOINTS][9];
  double joint_axis[RMPC_MAX_JOINTS][3];
  /* offsets into one stage's parameter slice (paramMap.yaml), -1 = absent */
  int32_t off_r_body, off_obst, off_lin, off_lower, off_upper, off_lower_u,
      off_upper_u, off_lower_vel, off_upper_vel, off_wu, off_goal, off_wgoal,
      off_wconstr, off_ws;
  int32_t has_goal, has_avoid;
  double lb[RMPC_NV_MAX], ub[RMPC_NV_MAX]; /* z bounds, +-inf allowed (mpcModel.py:91-104) */
  /* solver options.  A zeroed field means its default -- with ONE exception, acc_iters, where zero means off.  The stop
   * tests of an iteration come in this order: converged (exitflag 1), acceptable (2), iteration limit (0); an instance
   * that converges at iteration max_iter returns 1. */
  int32_t max_iter;     /* iteration limit, default 200; <= 0 means the default (NOT zero iterations) */
  double tol_stat, tol_eq, tol_ineq, tol_comp;  /* converged: stationarity, dynamics, inequality and complementarity
                           residuals (defaults 1e-6, 1e-8, 1e-8, 1e-6); each <= 0 or NaN means its default.  tol_comp
                           also sets the floor of the barrier parameter, 0.1 tol_comp */
  double mu0;           /* initial barrier parameter of a cold start (default 1.0); <= 0 or NaN means the default */
  int32_t acc_iters;    /* acceptable termination: consecutive stagnant feasible iterations (0 = off, default 8).  A
                           zeroed field is OFF, not 8: ask for the default by writing 8.  Negative values are off too */
  double acc_obj_tol;   /* ... relative objective change (default 1e-8); <= 0 or NaN means the default */
  int32_t ls_max;       /* step halvings allowed in one line search (default 25; <= 0 means the default); an instance
                           that exhausts them stops with exitflag -8 and its current iterate.  Small values bound the
                           number of passes of a real-time solve (examples/fleet_loop.py) */
  /* ---- 0.2.1: rows of the RMPC_MOD_ROWS modules, in row order; xrow_mod = index into module_kind.  The rows of one
   * module must all be on states (RADIAL / LINEAR / SELF, VAR with a < nx) or all on inputs (VAR with a >= nx + ns): the
   * stage-1 neutralisation and the inverse-barrier objective are per module (InequalityManager.py:25-33).  RADIAL and
   * LINEAR rows address their parameters as entries of the obstacle / plane lists: xrow_poff - off_obst (off_lin) must
   * be a multiple of 4 in [0, 252] (an absent list starts at the first such row). */
  int32_t n_xrows;
  int32_t xrow_mod[RMPC_MAX_XROWS];
  int32_t xrow_kind[RMPC_MAX_XROWS];
  int32_t xrow_a[RMPC_MAX_XROWS];
  int32_t xrow_b[RMPC_MAX_XROWS];
  int32_t xrow_poff[RMPC_MAX_XROWS];
} rmpc_desc;

typedef struct rmpc_handle rmpc_handle;

int rmpc_version(void);
/* sha256 (first 16 hex digits) of the sources this binary was built from (the files listed in
 * csrc/sources.txt, this header among them), embedded by __graft_entry__.build(); the Python binding
 * refuses a library whose hash differs from the sources next to it. */
const char *rmpc_source_hash(void);
const char *rmpc_last_error(void);
int rmpc_desc_size(void);

/* Replaces forcespro.nlp.Solver.from_directory (mpcPlanner.py:73): validates
 * the descriptor, selects the device and allocates the HBM workspace for up to
 * max_batch instances. */
int rmpc_create(const rmpc_desc *desc, int max_batch, rmpc_handle **out);
void rmpc_destroy(rmpc_handle *h);

/* Replaces solver.solve(problem) (mpcPlanner.py:262) for B instances; host
 * pointers, blocks until the results are in host memory. */
int rmpc_solve_batch(rmpc_handle *h, int B, const double *xinit, const double *x0,
                     const double *params, double *z_out, int32_t *exitflag,
                     int32_t *iters, double *kkt_res, double *obj);

/* Same, device pointers (e.g. torch tensor data_ptr()).  All work is enqueued on `stream`
 * (a hipStream_t; NULL = the legacy null stream, i.e. ordered with the caller's default-stream
 * work such as the torch ops that produced the inputs).  Returns when the iteration loop has
 * drained and the final kernel (the one that writes d_z_out ... d_obj) is ENQUEUED: the outputs
 * are valid for later work on the same stream, or for the host after a stream synchronize. */
int rmpc_solve_batch_device(rmpc_handle *h, int B, const double *d_xinit,
                            const double *d_x0, const double *d_params,
                            double *d_z_out, int32_t *d_exitflag, int32_t *d_iters,
                            double *d_kkt_res, double *d_obj, void *stream);

/* Warm start of the multipliers for closed loops (no counterpart in the reference, which warm-starts the plan
 * only: setX0 / shiftHorizon, mpcPlanner.py:215-236).  mode 1: a solve of B instances that follows a finished solve
 * of the same B instances on this handle starts instance b from the multipliers of ITS previous solve, shifted by one
 * stage like the plan (lambda_k <- lambda_{k+1}, nu_k <- nu_{k+1}, last stage repeated), with mu = clamp(1000 *
 * previous final mu, 1e-6, mu0), slacks t = max(g(x0), 1e-4) and lambda = max(previous, mu / t); an instance whose
 * previous solve failed starts from zero multipliers and mu0.  mode 0 (default): every solve starts cold.  Changing the mode, or solving another
 * batch size, forgets the stored multipliers. */
int rmpc_set_warm_start(rmpc_handle *h, int mode);

/* Real-time deadline of a solve, in passes (0 = none, the default).  A pass is one evaluation of the whole horizon:
 * the start point, every trial point of a line search, every step recomputed with the Gauss-Newton blocks -- the
 * unit the device pays for (an iteration costs one pass plus one per backtracking).  An instance still iterating
 * when the budget is spent returns its last accepted iterate with exit flag 0, exactly as at the iteration limit;
 * instances that finish earlier are unaffected.  No reference counterpart (FORCES Pro offers a wall-clock
 * `solver_timeout`); used by the fleet loop, where a few instances in hopeless states would otherwise hold the
 * control step of thousands.  Budgets below max_iter + 1 also bound the iterations. */
int rmpc_set_pass_budget(rmpc_handle *h, int passes);

/* 1 when the solves of this handle run as ONE launch that needs no look from the host (k_fused: point robot and
 * diff-drive base, N <= 32) -- rmpc_solve_batch_device then only enqueues work on the stream and returns; 0 when they
 * run as pass kernels, whose host loop reads a counter every few passes and returns when the batch is done. */
int rmpc_is_fused(const rmpc_handle *h);
/* the kernel behind a fused handle: "k_fused" (point robot, diff-drive base: two instances per wavefront, lane = stage),
 * "k_fused_arm" (arms with 5 .. 7 joints: one instance per wavefront, a stage per two lanes), "" for the pass kernels */
const char *rmpc_fused_kernel_name(const rmpc_handle *h);

/* 1 when rmpc_solve_batch_device (and the scene / packed variants) of this handle only ENQUEUES work on the stream and
 * returns -- no look from the host, the solve is ordered with the caller's stream like any kernel: fused handles
 * always, handles on the pass kernels (the arm, N > 32) when a pass budget is set (the budgeted passes are enqueued
 * whole; kernels leave at once when no instance iterates any more).  Without a budget the pass kernels' host loop
 * reads a counter every few passes, because only it can know how many passes to enqueue (a solve then returns when
 * the batch is done; the reference's solver.solve() is synchronous too, mpcPlanner.py:262). */
int rmpc_is_async(const rmpc_handle *h);

/* Workspace size in bytes for a given descriptor / batch (no allocation). */
int64_t rmpc_workspace_bytes(const rmpc_desc *desc, int max_batch);

/* Per-kernel timing with HIP events on the solver's stream.
 * kernels: 0 pack, 1 sweep, 2 riccati, 3 step, 4 unpack (pass kernels: large horizons, the arm),
 * 5 fused (whole solves inside one wavefront, N <= 32: point robot, diff-drive base, arms with 5 .. 7 joints --
 *   rmpc_fused_kernel_name tells which kernel). */
#define RMPC_NUM_KERNELS 6
int rmpc_set_profiling(rmpc_handle *h, int enable);
/* total_ms / launches: summed HIP-event durations and launch counts per kernel;
 * total_alg_bytes: algorithmic bytes of those launches, counting only the lanes
 * that were still active in each launch; full_launch_bytes: algorithmic bytes
 * of one launch with every lane of a max_batch batch active. */
int rmpc_get_profile(rmpc_handle *h, double *total_ms, int64_t *launches,
                     double *total_alg_bytes, int64_t *full_launch_bytes);
const char *rmpc_kernel_name(int idx);
/* number of sweep/riccati/step passes of the last solve, and instance-iterations */
int rmpc_last_passes(rmpc_handle *h);

/* ---- next rows of the hot path: inputs produced on the device ---------- */

/* Compact scene of B instances; every pointer is a DEVICE pointer and may be NULL.  A NULL field is left at zero, with
 * one exception, the obstacle words of a model that has them: when BOTH obst and obst_dyn are NULL every obstacle word
 * (position and radius of all nobst slots) is -100, the reference's EmptyObstacle (mpcPlanner.py:18-26,127-133), as the
 * host packer's setRadialConstraints writes them for obstacles not given.  When both are given obst_dyn wins: the
 * predicted obstacles are written and obst is not read.  A field the model has no parameter for is not read.
 * Device counterpart of MPCPlanner.reset() + setGoalReaching / setRadialConstraints /
 * setLinearConstraints / setJointLimits / setInputLimits / setVelLimits / setConstraintAvoidance /
 * updateDynamicObstacles (robotmpcs/planner/mpcPlanner.py:83-210). */
typedef struct rmpc_scene {
  int32_t struct_size;        /* sizeof(rmpc_scene) */
  const double *goal;         /* [B][3]            setGoalReaching, zero padded (:197-204) */
  const double *r_body;       /* [B]               (:122,137,165) */
  const double *obst;         /* [B][nobst][4]     static obstacles: position, radius (:120-133) */
  const double *obst_dyn;     /* [B][nobst][9]     position, velocity, acceleration; stage k predicted at dt*k (:144-161) */
  double dyn_radius;          /*                   radius of the predicted obstacles, self._r = 0.1 (:121) */
  const double *lower_limits, *upper_limits;         /* [B][n]   (:167-175) */
  const double *lower_limits_u, *upper_limits_u;     /* [B][nu]  (:187-195) */
  const double *lower_limits_vel, *upper_limits_vel; /* [B][2]   (:177-185) */
  const double *lin_constrs;  /* [B][N][nobst][4]  planes per stage (:135-141) */
  double w, wu, ws;           /*                   weights["w"], ["wu"], ["ws"], broadcast by reset() (:92-104) */
  double wconstr[RMPC_MAX_MODULES]; /*             weights["wconstr"] (:206-210) */
} rmpc_scene;

/* all_parameters [B][N][npar] (ABI layout) from a scene; bit-identical to the host packer. */
int rmpc_pack_scene_device(rmpc_handle *h, int B, const rmpc_scene *scene, double *d_params, void *stream);

/* rmpc_solve_batch_device with the parameters expanded from a scene straight into the solver's
 * workspace: the B*N*npar array never exists in the ABI layout. */
int rmpc_solve_batch_scene_device(rmpc_handle *h, int B, const rmpc_scene *scene, const double *d_xinit,
                                  const double *d_x0, double *d_z_out, int32_t *d_exitflag, int32_t *d_iters,
                                  double *d_kkt_res, double *d_obj, void *stream);

/* The two halves of rmpc_solve_batch_scene_device, for callers that drive several handles on several streams: the
 * packing kernels of all of them can be enqueued before the first solve (a fused solve fills every SIMD for
 * milliseconds; a small kernel enqueued behind it on another stream waits for a free slot first).
 * rmpc_solve_batch_packed_device solves with the parameters rmpc_pack_scene_workspace left in the workspace (same
 * handle, same B, same stream). */
int rmpc_pack_scene_workspace(rmpc_handle *h, int B, const rmpc_scene *scene, void *stream);
int rmpc_solve_batch_packed_device(rmpc_handle *h, int B, const double *d_xinit, const double *d_x0, double *d_z_out,
                                   int32_t *d_exitflag, int32_t *d_iters, double *d_kkt_res, double *d_obj, void *stream);

/* Closed loop between two solves, on the device: xinit <- Phi(xinit, u_1 of the previous plan)
 * with the model's own ERK2 map (the plant of the examples' env.step), and the warm start
 * x0 <- shifted plan (shiftHorizon, mpcPlanner.py:215-226) when previous_plan != 0, else the new
 * state repeated over the horizon with zero controls (setX0 "current_state", :228-232). */
int rmpc_advance_device(rmpc_handle *h, int B, const double *d_z_prev, double *d_xinit, double *d_x0,
                        int previous_plan, void *stream);
/* The same with the exit flags of the solve that produced d_z_prev ([B], device): an instance whose solve failed
 * (exitflag < 0) restarts from its new state ("current_state" initialisation) whatever previous_plan says -- the
 * closed-loop fallback of the reference's boxer example (examples/boxer_example.py:194-198). */
int rmpc_advance_device_flags(rmpc_handle *h, int B, const double *d_z_prev, const int32_t *d_exitflag, double *d_xinit,
                              double *d_x0, int previous_plan, void *stream);

/* Steady closed loop (fleet harness; the examples of the reference hand the planner its next goal whenever the driver
 * has one -- setGoalReaching every control step with the next waypoint, examples/boxer_example_global.py:203-212).
 * Called after rmpc_advance_device_flags, once per control step.  Every pointer is a DEVICE pointer.
 *  - an instance whose end link is within `tol` of its goal has ARRIVED; one that has come to rest (largest joint /
 *    wheel speed below settle_vel after at least settle_min_dwell control steps on this goal; settle_vel = 0: off) has
 *    SETTLED -- with the reference's objective (N w / h on the first row of a module, constraint_avoidance.py:22-31) a
 *    goal next to an obstacle is an equilibrium at a distance, not a point that is reached; one that has spent
 *    max_dwell control steps on its goal (0: no limit) has TIMED OUT.  All three take the next goal of their pool
 *    goal_pool [B][pool_len][3] (cursor [B], dwell [B]: int32, zero-initialised by the caller).
 *  - an instance whose solve FAILED (exitflag < 0) keeps its state: the reference prints the flag and applies the action
 *    it got (mpcPlanner.py:263-264), the next solve starts cold from the new state (rmpc_advance_device_flags =
 *    examples/boxer_example.py:194-198).  Only after fail_reset_after failed control steps IN A ROW (failrun [B], int32,
 *    zero-initialised; 0: never) is it put back to x_start [B][nx] with a cold plan and its next goal: a RESET.  The same
 *    happens at once to an instance whose configuration has left the joint-limit box lower_limits / upper_limits [B][n]
 *    (may be NULL: no check) by more than 5 % of its width: the plant of the loop is the bare integrator, the examples'
 *    simulator would have stopped the joint at its limit (counted in counts[12] as well).
 *  - mu_regoal > 0 (with rmpc_set_warm_start(1)): the next solve of an instance that has just taken a new goal keeps its
 *    multipliers but restarts its barrier parameter from mu_regoal; 0: plain warm start.
 *  - goal [B][3] is the array the scene (rmpc_scene.goal) points at.
 *  - counts (may be NULL): sixteen int64 counters, incremented: [0] arrivals, [1] settled, [2] time-outs, [3] resets,
 *    [4..7] the control step's exit flags (1, 2, 0, < 0), [8] sum of iters (may be NULL), [9] sum of the distance to the
 *    goal at the hand-overs in micrometres, [10] hand-overs counted in [9], [11] instances inside a run of failed
 *    solves this step, [12] resets because the robot had left its workspace, [13..15] reserved (never written) -- loop
 *    statistics without a host read per control step (64-bit: a loop may run for days).
 *  The order of one call, per instance (tests/steady_loop_reference.py restates it in numpy):
 *   1. the fail run: failrun + 1 when exitflag < 0, else 0 (exitflag NULL: nothing has failed; failrun NULL: the run
 *      before this step counts as 0, so only fail_reset_after = 1 can fire).
 *   2. RESET when a joint q_j < lo_j - 0.05 (hi_j - lo_j) or q_j > hi_j + 0.05 (hi_j - lo_j) (strict; counts[12]), or
 *      when the solve failed and the fail run has reached fail_reset_after (>=).  A reset writes x_start to xinit and
 *      to the state part of every stage of x0, zeroes the slack and control part of x0, and ends the fail run (0).
 *      counts[11] counts the instances whose fail run is > 0 AFTER this, so an instance that is reset is not in it.
 *   3. distance (end frame of the descriptor at q = x[0..n) to goal) and speed (chain: max |x[n + j]|, j < n;
 *      diff-drive base: max(|x[6]|, |x[7]|)) are taken from the state after step 2 (x_start for a reset instance), the
 *      goal is the one before the hand-over.  dwell + 1 is the
 *      number of control steps on this goal.  ARRIVED: distance < tol (strict).  SETTLED: not arrived, settle_vel > 0,
 *      dwell + 1 >= settle_min_dwell and speed < settle_vel (strict).  TIMED OUT: max_dwell > 0 and dwell + 1 >=
 *      max_dwell.
 *   4. any of the four hands over: cursor + 1, goal = goal_pool[b][cursor mod pool_len] (cursor itself is not
 *      wrapped), dwell = 0; otherwise dwell + 1 is stored and xinit, x0 and goal are not written.  A hand-over is
 *      counted ONCE, for the first that holds of: reset [3], arrived [0], settled [1], timed out [2].  counts[9] and
 *      [10] take the hand-overs that are not resets (the distance truncated to whole micrometres).
 *   5. mu_regoal applies to every hand-over, a reset included, unless exitflag < 0 this step (the next solve of a
 *      failed instance keeps the barrier parameter the failed solve left for it).
 *  [4..8] are counted only when both counts and exitflag are given; flags other than 1, 2, 0 and < 0 are in no class. */
typedef struct rmpc_retarget {
  int32_t struct_size;            /* sizeof(rmpc_retarget) */
  int32_t pool_len;
  double *xinit, *x0;             /* [B][nx], [B][N][nvar] */
  const int32_t *exitflag, *iters;
  double *goal;
  const double *goal_pool, *x_start;
  const double *lower_limits, *upper_limits;
  int32_t *cursor, *dwell, *failrun;
  double tol, settle_vel, mu_regoal;
  int32_t settle_min_dwell, max_dwell, fail_reset_after, reserved;
  int64_t *counts;
} rmpc_retarget;
int rmpc_retarget_device(rmpc_handle *h, int B, const rmpc_retarget *r, void *stream);

/* The moving obstacles between two control steps (what the examples' simulator does before the driver hands the planner
 * ob[nx:], mpcPlanner.py:243-244): d_obst_dyn [B][nobst][9] = position, velocity, acceleration (rmpc_scene.obst_dyn):
 * pos += vel dt + acc dt^2 / 2, vel += acc dt.  arena > 0: an obstacle that leaves [-arena, arena] in x or y comes back
 * with that velocity component mirrored.  Needs no handle. */
int rmpc_advance_obstacles_device(int B, int nobst, double dt, double arena, double *d_obst_dyn, void *stream);

/* Free-space decomposition on the device: for each of the B*N seed points
 * (e.g. the planned lidar position of instance b at stage k) at most K half-planes
 * [a(3), d] from instance b's point cloud of P <= 64 points, greedy nearest-point rule and dummy
 * planes of robotmpcs/utils/free_space_decomposition.py:79-116.  d_points [B][P][3],
 * d_seeds [B][N][3], d_planes [B][N][K][4] = the lin_constrs field of rmpc_scene
 * (setLinearConstraints, mpcPlanner.py:135-141; called N times per control step by
 * examples/boxer_example.py:193-203).  Needs no handle; runs on the device of d_points. */
int rmpc_free_space_device(int B, int N, int P, int K, double max_radius, const double *d_points,
                           const double *d_seeds, double *d_planes, void *stream);

/* Global planner on the device (robotmpcs/global_planner/: globalPlanner.py, a_star.py, gridmap.py).  Needs no handle;
 * every pointer is a device pointer, each call runs on the device of its first pointer.  A grid is d_grid [H][W]
 * doubles, row-major, cell c = row * W + col; in the plain frame the centre of (row, col) is (x0 + col cell,
 * y0 + row cell) (gridmap.py:get_coordinates_from_index with an origin).  A cell is occupied when data >= occ_threshold
 * (OccupancyGridMap, 0.8); entering cell v costs delta + cost_factor data[v], delta = 1 axial, sqrt(2) diagonal
 * (a_star.py:99-116, occupancy_cost_factor 3); movement 8 or 4 takes the reference's move order
 * (_get_movements_8n / _get_movements_4n; diagonal steps between two occupied cells are allowed, as there). */
#define RMPC_GRID_MAX_CELLS 16384       /* one cost-to-go field per workgroup, held in LDS: 128 x 128 */
#define RMPC_GRID_OK 0
#define RMPC_GRID_START_OCCUPIED (-1)   /* a_star.py:55-56 raises */
#define RMPC_GRID_GOAL_OCCUPIED (-2)    /* a_star.py:58-59 raises */
#define RMPC_GRID_OUTSIDE (-3)          /* gridmap.py:is_occupied_idx raises; also a goal index outside [0, G) */
#define RMPC_GRID_TOO_LONG (-4)         /* the path has more than max_len cells */
#define RMPC_GRID_BAD_MAP (-5)          /* a free cell (data < occ_threshold) holds a negative value */
#define RMPC_GRID_NO_FIXED_POINT (-6)   /* no fixed point after H W + 1 sweeps (not reached with prices >= 0) */
#define RMPC_GRID_BAD_SEED (-7)         /* rmpc_grid_fields_seeded_device: a free cell holds a negative or NaN seed */

/* get_enlarged_obstacles (globalPlanner.py:39-70): box mean over (2k+1)^2 cells, k = ceil(size_robot / cell), on the
 * cells at least k from the border (convolution_size_robot; the others keep their raw value), then 1 where the value is
 * above threshold (0.29 in the reference) and 0 elsewhere.  d_out [H][W] may not alias d_grid. */
int rmpc_grid_inflate_device(int H, int W, double cell, double size_robot, double threshold, const double *d_grid,
                             double *d_out, void *stream);
/* One cost-to-go field per goal cell d_goal_cells [G]: d_fields [G][H][W], D(goal) = 0,
 * D(u) = min_v (delta(u,v) + cost_factor data[v] + D(v)), +inf on occupied and unreachable cells -- the exact fixed
 * point, bitwise the same on every run.  d_status [G]: RMPC_GRID_OK, _GOAL_OCCUPIED, _OUTSIDE, _BAD_MAP or
 * _NO_FIXED_POINT (field all +inf).  cost_factor must be finite and >= 0 (prices may not be negative: refused).
 * d_sweeps [G] (may be NULL): the sweeps the field took.  H W <= RMPC_GRID_MAX_CELLS, larger maps are refused
 * (rmpc_grid_large.h has the entries that take them). */
int rmpc_grid_fields_device(int H, int W, const double *d_grid, int G, const int32_t *d_goal_cells, int movement,
                            double occ_threshold, double cost_factor, double *d_fields, int32_t *d_status,
                            int32_t *d_sweeps, void *stream);
/* One path per query: from d_start_cell [b] down field d_goal_index [b] (neighbour with the least delta +
 * cost_factor data[v] + D(v), the first in move order on ties) to its goal.  d_path [B][max_len] int32 cells with start
 * and goal; d_len [B] > 0 the path's cell count, 0 the goal is unreachable (a_star.py:119-133 returns empty lists),
 * or RMPC_GRID_START_OCCUPIED, _GOAL_OCCUPIED, _OUTSIDE, _TOO_LONG.  Cells past d_len [b] are not written. */
int rmpc_grid_paths_device(int H, int W, const double *d_grid, int G, const double *d_fields, const int32_t *d_goal_cells,
                           int B, const int32_t *d_start_cell, const int32_t *d_goal_index, int movement,
                           double occ_threshold, double cost_factor, int max_len, int32_t *d_path, int32_t *d_len,
                           void *stream);
/* Fields to a set of cells: as rmpc_grid_fields_device, but field g takes its sources from
 * d_seeds [g][H][W] instead of one goal cell: D(u) = min(seed(u), min_v (delta(u,v) + cost_factor data[v] + D(v))), +inf
 * on occupied and unreachable cells -- the distance to the nearest source, the exact fixed point, bitwise the same on
 * every run.  A seed is +inf (no source) or finite and >= 0: 0 an ordinary source, a positive one a start potential that
 * prices the source; a neighbour may undercut it.  A seed on an occupied cell is ignored.  With seed 0 at one free cell
 * and +inf elsewhere the field is that of rmpc_grid_fields_device for that goal, bit for bit.  d_status [G]:
 * RMPC_GRID_OK (also for a field without a finite seed: all +inf), _BAD_MAP, _NO_FIXED_POINT, or RMPC_GRID_BAD_SEED when a
 * free cell holds a negative or NaN seed (field all +inf, sweeps 0); the other fields of the launch are not affected.
 * Arguments are refused as by rmpc_grid_fields_device. */
int rmpc_grid_fields_seeded_device(int H, int W, const double *d_grid, int G, const double *d_seeds, int movement,
                                   double occ_threshold, double cost_factor, double *d_fields, int32_t *d_status,
                                   int32_t *d_sweeps, void *stream);
/* One path per query down a seeded field: from d_start_cell [b] down field d_field_index [b] of d_fields [G][H][W]
 * (built from d_seeds [G][H][W] on d_grid) by the step rule of rmpc_grid_paths_device, until the first cell u with D(u)
 * finite and D(u) == seed(u): a source that nothing undercuts.  A source whose seed a neighbour undercuts is passed
 * through.  The start cell is exempt from the occupancy test (a robot stands where it stands): from a start with
 * D = +inf the first step goes to the best free neighbour.  d_path [B][max_len] int32 cells with start and source;
 * d_len [B] > 0 the path's cell count (1: the start is a source), 0 no neighbour of such a start has a finite D (or the
 * start cannot reach a source), or RMPC_GRID_OUTSIDE (the start or the field index), RMPC_GRID_TOO_LONG.  Cells past
 * d_len [b] are not written.  The loop is bounded by max_len.  Arguments are refused as by rmpc_grid_paths_device. */
int rmpc_grid_descend_device(int H, int W, const double *d_grid, int G, const double *d_fields, const double *d_seeds,
                             int B, const int32_t *d_start_cell, const int32_t *d_field_index, int movement,
                             double occ_threshold, double cost_factor, int max_len, int32_t *d_path, int32_t *d_len,
                             void *stream);
/* World positions d_pos [b * stride + 0 .. 1] (e.g. xinit [B][nx], stride nx) to cells d_cells [B] of the plain frame,
 * rint((p - origin) / cell) (round half to even, gridmap.py:get_index_from_coordinates); -1 outside the map. */
int rmpc_grid_cells_device(int B, const double *d_pos, int stride, int H, int W, double x0, double y0, double cell,
                           int32_t *d_cells, void *stream);
/* get_local_goal (globalPlanner.py:174-189) for B robots in one control step: when d_idx [b] < d_len [b] - 1 and the
 * distance from d_pos [b * stride + 0 .. 1] to the centre of d_path [b][d_idx [b]] is <= threshold (1.3 m in the
 * reference), d_idx [b] advances by one; then d_goal [b] = (centre of d_path [b][d_idx [b]], 0) -- the goal [B][3] the
 * scene points at (rmpc_scene.goal, rmpc_retarget.goal).  Robots with d_len [b] <= 0 keep their goal. */
int rmpc_follow_path_device(int B, const int32_t *d_path, const int32_t *d_len, int max_len, int32_t *d_idx,
                            const double *d_pos, int stride, int W, double x0, double y0, double cell, double threshold,
                            double *d_goal, void *stream);

/* Lidar on the device (the Lidar sensor and compute_point_cloud of examples/boxer_example_supermarket.py).  Needs no
 * handle; every pointer is a device pointer, each call runs on the device of its first pointer.  B robots scan one
 * world of axis-aligned boxes [nbox][4] = (cx, cy, lx, ly) (BoxObstacle position, length along x, width along y) and
 * circles [ncircle][3] = (cx, cy, r).  Robot b has the pose (x, y, th) = pose [b * pose_stride + 0 .. 2]; its sensor
 * sits at o = (x + offset_x cos th - offset_y sin th, y + offset_x sin th + offset_y cos th) (the boxer: (0.4, 0)).
 * Ray i of R has the angle th + angle_min + i (angle_max - angle_min) / R (half-open: [-pi, pi) is a full circle)
 * and the direction d = (cos, sin).  A box is hit at its entering distance 0 < t_enter <= t_exit (slab test; a
 * direction component of exactly 0 is inside its slab iff the origin coordinate lies in the closed interval), a circle
 * at t = -b - sqrt(b^2 - c), b = d.(o - c), c = |o - c|^2 - r^2, when c > 0, b^2 - c >= 0 and t > 0.  A shape that
 * contains the origin is ignored by that ray.  t is the least hit distance, range when nothing is hit within range.
 * points [B][R][3] = (o + t d, height): the absolute cloud of compute_point_cloud, laid out as the d_points of
 * rmpc_free_space_device; ranges [B][R] = t (may be NULL).  The convention is the project's own.
 * struct_size must equal sizeof(rmpc_lidar); refused (-1, rmpc_last_error): NULL pointers where a count is
 * positive, B < 1, rays < 1, pose_stride < 3, a negative shape count, a range that is not positive and finite, and
 * B*rays, nbox*4 or ncircle*3 beyond INT_MAX. */
typedef struct rmpc_lidar {
  int32_t struct_size;                 /* sizeof(rmpc_lidar) */
  int32_t rays;                        /* R >= 1 */
  double angle_min, angle_max, range;  /* body frame; range > 0 */
  double offset_x, offset_y, height;
  const double *pose; int32_t pose_stride;     /* [B][stride]: x, y, heading at 0, 1, 2 (xinit: stride nx) */
  int32_t nbox; const double *boxes;           /* [nbox][4] */
  int32_t ncircle; const double *circles;      /* [ncircle][3] */
  double *points;                              /* [B][R][3] out */
  double *ranges;                              /* [B][R] out, may be NULL */
} rmpc_lidar;
int rmpc_lidar_scan_device(int B, const rmpc_lidar *l, void *stream);
/* The fleet in the scan: the scan of l plus P round bodies, one per robot of the fleet, so that the
 * robots see each other.  Ray (b, i): origin o, direction d and the static hit distance ts are exactly those of
 * rmpc_lidar_scan_device on l (the same expressions in the same order).  Body j = (centres [j * centre_stride + 0 .. 1],
 * radius [j]) is a candidate when j != self0 + b (the scanning robot's own body) and radius [j] > 0; a candidate is
 * tested by the circle rule above: u = o - c_j, bb = d.u, cc = |u|^2 - r^2, disc = bb^2 - cc, a hit iff cc > 0,
 * disc >= 0 and tc = -bb - sqrt(disc) > 0.  A body that contains the origin is ignored, as any shape is; a NaN centre
 * or radius never hits.  t is the least of ts and all tc; a body replaces the static world only when tc < ts strictly,
 * and among bodies the least (tc, j) wins: nothing depends on the order in which the bodies are met.
 * points and ranges of l are as in the plain scan, with this t; static_ranges = ts; owner = j when a body gave t, -2 when
 * a box or a circle of l did, -1 when t == range.  P == 0 gives the plain scan's result.
 * Runs on the device of l->pose, on the given stream, and never synchronises.  struct_size must equal
 * sizeof(rmpc_lidar_bodies); refused (-1, rmpc_last_error): everything rmpc_lidar_scan_device refuses, P < 0, NULL
 * centres or radius with P > 0, centre_stride < 2, and P*centre_stride beyond INT_MAX. */
typedef struct rmpc_lidar_bodies {
  int32_t struct_size;                 /* sizeof(rmpc_lidar_bodies) */
  int32_t P;                           /* bodies, >= 0 */
  const double *centres; int32_t centre_stride;  /* [P][stride >= 2]: cx, cy at 0, 1 (rmpc_fleet_points_device, N = 1: stride 3) */
  const double *radius;                /* [P] */
  int32_t self0;                       /* scanning robot b is body self0 + b (outside [0, P): it has none) */
  int32_t *owner;                      /* [B][R] out, may be NULL */
  double *static_ranges;               /* [B][R] out, may be NULL */
} rmpc_lidar_bodies;
int rmpc_lidar_scan_fleet_device(int B, const rmpc_lidar *l, const rmpc_lidar_bodies *f, void *stream);
/* The seeds of the free-space decomposition (examples/boxer_example_supermarket.py, "Preprocessing for planner"):
 * d_points [B][N][3] = (sensor origin of q, height) with q = d_z_prev [b][k][0 .. 2] (stage k of the previous plan,
 * [B][N][nvar] with z_k = [x_k; s_k; u_k]), or q = the current pose d_pose [b * pose_stride + 0 .. 2] when d_z_prev is
 * NULL (first control step) or d_exitflag [b] < 0 (d_exitflag may be NULL).  The same offset and height as the scan;
 * the seeds are not shifted (the reference's lag of one control step).  Runs on the device of d_z_prev, of d_pose when
 * d_z_prev is NULL.  Refused: NULL d_pose or d_points, B < 1, N < 1, pose_stride < 3, nvar < 3, and B*N,
 * B*pose_stride or B*N*nvar beyond INT_MAX. */
int rmpc_plan_points_device(int B, int N, const double *d_z_prev, int nvar, const int32_t *d_exitflag,
                            const double *d_pose, int pose_stride, double offset_x, double offset_y, double height,
                            double *d_points, void *stream);

/* The map from the fleet's scans: evidence in two int32 grids d_hits [H][W] and d_misses [H][W] in the
 * plain frame of the global planner (cell (row, col) centred at (x0 + col cell, y0 + row cell)), and the occupancy
 * grid classified from them.  Needs no handle; every pointer is a device pointer, each call runs on the device of its
 * first pointer (origins, d_hits).  The counts are integers: the map does not depend on the order of the updates and is
 * bitwise the same on every run.
 * rmpc_grid_mark_device ADDS one scan of B robots to hits and misses.  origins [B][3]: the sensor origins, the output
 * of rmpc_plan_points_device with N = 1 and d_z_prev = NULL; points [B][rays][3] and ranges [B][rays]: the outputs of
 * rmpc_lidar_scan_device.  Ray (b, i) with o = origins [b][0 .. 1], e = points [b][i][0 .. 1], t = ranges [b][i], every
 * floating-point operation in the order written:
 *  1. the ray is skipped (and *skipped, when given, grows by 1) unless o, e and t are finite and 0 < t <= range;
 *  2. hit = t < range; if hit: s = hit_depth / t, ex <- ex + s (ex - ox), ey likewise (the scan's end point lies on the
 *     obstacle's face, in a world made by boxes_from_grid a cell edge: the end cell is taken hit_depth behind it);
 *  3. ua = (ox - x0) / cell + 0.5, va = (oy - y0) / cell + 0.5, ub, vb likewise from e; c = floor(ua), r = floor(va),
 *     c1 = floor(ub), r1 = floor(vb), n = |c1 - c| + |r1 - r|; the ray is skipped, counted as above, unless
 *     n <= 2 ceil((range + hit_depth) / cell) + 4 (a garbage point cannot run an unbounded loop; a cell coordinate that
 *     is not finite fails the test too);
 *  4. du = ub - ua, dv = vb - va, sc = du > 0 ? 1 : -1, tx = du != 0 ? ((c + (du > 0 ? 1 : 0)) - ua) / du : +inf; sr and
 *     ty likewise from dv, r, va;
 *  5. n + 1 cells are visited from (r, c): a visited cell inside [0, H) x [0, W) gets misses += 1, but the last cell of
 *     a ray with hit gets hits += 1; cells outside the map are passed over.  Between two visits the column steps
 *     (c += sc, tx recomputed from the new c) when (tx <= ty and c != c1) or r == r1, otherwise the row does.
 * This is the cell walk of Amanatides and Woo along o -> e; it ends on (r1, c1) and a ray visits a cell at most once.
 * The cell of a point is floor((p - origin) / cell + 0.5) here, rint((p - origin) / cell) (half to even) in
 * rmpc_grid_cells_device: the two differ only for a point exactly on a cell edge.
 * The counters wrap unguarded: the calls between two resets times B rays must stay below 2^31 (rmpc_grid_occupancy_device
 * with forget > 0 ages them).
 * struct_size must equal sizeof(rmpc_grid_mark); refused (-1, rmpc_last_error): NULL pointers other than skipped, B < 1,
 * rays < 1, H or W < 1, H W > RMPC_GRID_MAX_CELLS, a cell or range that is not positive and finite, a hit_depth that is
 * negative or not finite, x0 or y0 not finite, B rays 3 beyond INT_MAX, and (range + hit_depth) / cell beyond 2^29. */
typedef struct rmpc_grid_mark {
  int32_t struct_size;                 /* sizeof(rmpc_grid_mark) */
  int32_t rays;                        /* R >= 1 */
  const double *origins;               /* [B][3] */
  const double *points;                /* [B][R][3] */
  const double *ranges;                /* [B][R] */
  double range, hit_depth;             /* the scan's range (> 0); hit_depth >= 0 */
  int32_t H, W;
  double x0, y0, cell;
  int32_t *hits, *misses;              /* [H][W] in/out */
  int32_t *skipped;                    /* one counter in/out, may be NULL */
} rmpc_grid_mark;
int rmpc_grid_mark_device(int B, const rmpc_grid_mark *m, void *stream);
/* d_grid [H][W] from the evidence, one cell each: unknown_value when hits + misses == 0, occ_value when
 * (int64) hits w_hit > (int64) misses w_miss, free_value otherwise (equal weights of evidence: free).  Then, when
 * forget > 0, both counters are shifted right by forget bits: ageing, which bounds the counters of a long loop and
 * lets an obstacle that moved fade.  The three values are the caller's (68/256 free and 253/256 occupied are what
 * rmpc_grid_inflate_device gets in the reference's PNG round trip).  Refused: NULL pointers, H or W < 1,
 * H W > RMPC_GRID_MAX_CELLS, w_hit or w_miss < 1, forget outside [0, 31], a value that is not finite. */
int rmpc_grid_occupancy_device(int H, int W, int32_t *d_hits, int32_t *d_misses, int w_hit, int w_miss, int forget,
                               double free_value, double occ_value, double unknown_value, double *d_grid, void *stream);
/* The frontier of the map, one cell each, from the evidence d_hits, d_misses [H][W] and d_enlarged
 * [H][W], the output of rmpc_grid_inflate_device on an occupancy grid whose unknown cells got the free value:
 *   known(c)    = hits[c] + misses[c] != 0                       (the rule of rmpc_grid_occupancy_device)
 *   d_plan[c]   = known(c) ? d_enlarged[c] : unknown_value       (the unknown region is not dilated; with
 *                 unknown_value >= occ_threshold routes stay inside what has been seen)
 *   frontier(c) = known(c) && d_enlarged[c] < occ_threshold && a neighbour of c inside the map is not known
 *                 (nmoves 4 or 8: the first nmoves moves of the planner's order; the map's edge is not unknown)
 *   d_seed[c]   = frontier(c) ? 0 : +inf                         (the d_seeds of rmpc_grid_fields_seeded_device)
 * and *d_count grows by the number of frontier cells (int32 adds, independent of their order; the caller zeroes it).
 * Runs on the device of d_hits.  Refused: NULL pointers, H or W < 1, H W > RMPC_GRID_MAX_CELLS, nmoves other than 4
 * or 8, an occ_threshold or unknown_value that is not finite. */
int rmpc_grid_frontier_device(int H, int W, const int32_t *d_hits, const int32_t *d_misses, const double *d_enlarged,
                              double occ_threshold, int nmoves, double unknown_value, double *d_plan, double *d_seed,
                              int32_t *d_count, void *stream);

/* Coordinated exploration: distinct frontier targets for the robots of a fleet.  Needs no handle; every
 * pointer is a device pointer, each call runs on the device of its first pointer and never synchronises.  The chain is
 *   rmpc_grid_frontier_device -> rmpc_grid_targets_device -> rmpc_grid_fields_seeded_device (G = T, d_seeds = d_tseeds)
 *   -> rmpc_grid_route_costs_device -> rmpc_assign_greedy_device -> rmpc_grid_descend_device (d_field_index = d_assign,
 *   d_seeds = d_tseeds),
 * and a robot left with d_assign = -1 gets RMPC_GRID_OUTSIDE from the descent.  Every result is a minimum under a strict
 * total order, so none depends on the order in which the device's lanes meet.
 *
 * rmpc_grid_targets_device: one target per tile of the frontier.  The map is cut into tiles of tile x tile cells, edge
 * tiles smaller: T = ceil(H / tile) ceil(W / tile), cell (r, c) lies in tile (r / tile) ceil(W / tile) + c / tile.  A
 * source is a cell with d_seed [c] < +inf (d_seed [H][W]: the seed output of rmpc_grid_frontier_device).  For a tile
 * with n sources whose rows sum to Sr and columns to Sc, the target is the source that minimises
 * (n r - Sr)^2 + (n c - Sc)^2 in int64, the lower cell index on ties: the source nearest the centroid of the tile's
 * sources, in exact integer arithmetic.  d_target_cells [T] int32: that cell, -1 for a tile without a source.
 * d_tseeds [T][H][W] (may be NULL) is written completely: 0 at tile t's target, +inf on every other cell.  Refused:
 * NULL d_seed or d_target_cells, H or W < 1, H W > RMPC_GRID_MAX_CELLS, tile < 1, T > RMPC_ASSIGN_MAX_TARGETS.
 *
 * rmpc_grid_route_costs_device: d_cost [B][T] fp64, the cost of robot b's route to target t, from the seeded fields
 * d_fields [T][H][W] of d_grid [H][W].  With u = d_start_cell [b] and D = d_fields [t]: +inf when u lies outside
 * [0, H W); D(u) when that is finite; otherwise -- the robot stands on a cell the planning grid calls occupied, the
 * start rule of rmpc_grid_descend_device -- the least delta_m + (cost_factor d_grid [v] + D(v)), each operation
 * rounded as written, over the moves m (the first `movement`, 4 or 8) whose v = u + m lies inside the map with
 * d_grid [v] < occ_threshold, +inf when there is none.  Refused: NULL pointers, H or W < 1, a movement other than 4 or
 * 8, B outside [1, RMPC_ASSIGN_MAX_ROBOTS], T outside [1, RMPC_ASSIGN_MAX_TARGETS], T H W beyond INT_MAX, a cost_factor
 * that is negative or not finite.
 *
 * rmpc_assign_greedy_device: d_assign [B] int32, the target of every robot or -1, from any cost matrix d_cost [B][T]
 * (it knows nothing of grids); d_pass [B] int32 (may be NULL): the pass, counted from 0, in which the robot was taken,
 * or -1.  An entry is takeable when it is >= 0 and < +inf: NaN, negative and +inf entries are never taken.  The rule:
 *  1. all robots are free;
 *  2. a pass starts with every target available;
 *  3. within a pass, repeatedly: among free robots x available targets the takeable pair that is least by
 *     (cost, b, t), lexicographically, is assigned; its robot is no longer free, its target no longer available;
 *  4. the pass ends when no target is available or no takeable pair remains;
 *  5. if the pass assigned at least one robot and free robots remain, another pass starts;
 *  6. otherwise the rule stops; the robots still free get -1.
 * With B > T the targets are shared out round by round, with B <= T this is plain greedy matching.  The device takes
 * all pairs that are the least of their row and of their column at once, which gives this rule's result bit for bit
 * (DESIGN.md 16).  Refused: NULL d_cost or d_assign, B outside [1, RMPC_ASSIGN_MAX_ROBOTS], T outside
 * [1, RMPC_ASSIGN_MAX_TARGETS]. */
#define RMPC_ASSIGN_MAX_ROBOTS 4096
#define RMPC_ASSIGN_MAX_TARGETS 1024
int rmpc_grid_targets_device(int H, int W, const double *d_seed, int tile, int32_t *d_target_cells, double *d_tseeds,
                             void *stream);
int rmpc_grid_route_costs_device(int H, int W, const double *d_grid, int T, const double *d_fields, int B,
                                 const int32_t *d_start_cell, int movement, double occ_threshold, double cost_factor,
                                 double *d_cost, void *stream);
int rmpc_assign_greedy_device(int B, int T, const double *d_cost, int32_t *d_assign, int32_t *d_pass, void *stream);

/* Localisation: a pose estimate from a lidar scan and a map, by correlative scan matching (Olson 2009).
 * Needs no handle; every pointer is a device pointer, each call runs on the device of its first pointer (d_grid,
 * l->pose, m->pose), takes a stream and never synchronises.  The chain per control step is
 *   rmpc_lidar_project_device (the measured ranges at the believed pose) -> rmpc_scan_match_device,
 * against a table that rmpc_grid_edge_distance_device makes once per map.  Scores are int32 sums of table entries and
 * the choice is a minimum under a strict total order of integers: every result is bitwise the same on every run.
 *
 * rmpc_grid_edge_distance_device: the likelihood field as exact integers.  Every cell of d_grid [H][W] is cut into
 * sub x sub fine cells; fine cell (R, C) has the class d_grid [R / sub][C / sub] >= occ_threshold (a NaN is not
 * occupied).  d_d2 [H sub][W sub] int32 = min(cap, the least (R - R')^2 + (C - C')^2 over the fine cells (R', C') of the
 * other class inside the map), cap when there is none: the squared distance, in fine cells, to the nearest obstacle
 * face from either side (an end point inside a shelf is penalised like one short of it).  The map's edge is not a
 * face.  Refused: NULL pointers, H or W < 1, H W > RMPC_GRID_MAX_CELLS, sub outside [1, 8], cap outside [1, 65535], an
 * occ_threshold that is not finite.
 *
 * rmpc_lidar_project_device: the rmpc_lidar of a scan with ranges as an INPUT (must not be NULL); boxes and circles are
 * ignored.  points [b][i] = (o + t d, height) with t = ranges [b][i] and o, d formed from pose [b] exactly as
 * rmpc_lidar_scan_device forms them: with the scan's pose and the scan's ranges these are the scan's points bit for
 * bit, with a believed pose the scan as that pose would place it.  Refused as by rmpc_lidar_scan_device, except that
 * boxes and circles may be NULL whatever their counts, and a NULL ranges.
 *
 * rmpc_scan_match_device: per robot b with the prior (x, y, th) = pose [b * pose_stride + 0 .. 2], the points
 * [b][i][0 .. 1] = (px, py) projected at that prior and t = ranges [b][i]; every floating-point operation in the order
 * written:
 *  1. ray i is used iff t, px and py are finite and 0 < t < range (a hit); n = the number of used rays.  If
 *     n < min_hits: pose_out [b] = (x, y, th), best [b] = -1, score [b] = score0 [b] = 0, used [b] = n, and the robot is
 *     done (so is a robot with a NaN pose: its points are not finite);
 *  2. ux = px - x, uy = py - y;
 *  3. candidate (jth, jy, jx), 0 <= jth <= 2 nth, 0 <= jy, jx <= 2 nxy, with ith = jth - nth, iy = jy - nxy,
 *     ix = jx - nxy, has the index k = (jth (2 nxy + 1) + jy) (2 nxy + 1) + jx; with (c, s) = rot [jth] it places the
 *     ray's end at qx = (c ux - s uy) + (x + ix step_xy), qy = (s ux + c uy) + (y + iy step_xy): the scan turned about
 *     the robot's own position and shifted;
 *  4. C = floor(((qx - x0) / cell + 0.5) sub), R = floor(((qy - y0) / cell + 0.5) sub), compared as doubles: the ray
 *     costs d2 [R][C] when 0 <= R < H sub and 0 <= C < W sub, otherwise cap (a NaN fails the test); score(k) = the int32
 *     sum over the used rays;
 *  5. best [b] = the candidate that is least by (score, m, k), m = ix^2 + iy^2 + ith^2: ties go to the candidate
 *     nearest the prior, so a scan that tells nothing keeps the prior; score [b] = its score, score0 [b] the score of
 *     the centre candidate ix = iy = ith = 0; pose_out [b] = (x + ix step_xy, y + iy step_xy, th + ith step_th).
 * rot [2 nth + 1][2] = (cos, sin) of (j - nth) step_th comes from the caller, so that the device does only
 * * + - / floor and a host restatement that shares the table agrees bit for bit.  d2 [H sub][W sub] is the table of
 * rmpc_grid_edge_distance_device for the same cap (entries in [0, cap]), x0, y0, cell the map's plain frame.
 * struct_size must equal sizeof(rmpc_scan_match); refused (-1, rmpc_last_error): NULL pointers other than score0 and
 * used, B < 1, rays outside [1, RMPC_MATCH_MAX_RAYS], pose_stride < 3, min_hits < 1, a range that is not positive and
 * finite, H or W < 1, H W > RMPC_GRID_MAX_CELLS, sub outside [1, 8], cap outside [1, 65535], rays cap beyond INT_MAX, a
 * cell that is not positive and finite, x0 or y0 not finite, nxy or nth outside [0, 15], a step that is negative or
 * not finite, or 0 while its n is positive, and B rays 3 or B pose_stride beyond INT_MAX. */
#define RMPC_MATCH_MAX_RAYS 2048
typedef struct rmpc_scan_match {
  int32_t struct_size;                 /* sizeof(rmpc_scan_match) */
  int32_t rays;                        /* R in [1, RMPC_MATCH_MAX_RAYS] */
  const double *pose;                  /* [B][pose_stride]: the priors, x, y, heading at 0, 1, 2 */
  const double *points;                /* [B][R][3]: the scan projected at the priors */
  const double *ranges;                /* [B][R] */
  double range;                        /* the scan's range (> 0): t < range is a hit */
  int32_t pose_stride, min_hits;       /* >= 3; >= 1 */
  const int32_t *d2;                   /* [H sub][W sub] */
  int32_t H, W, sub, cap;
  double x0, y0, cell;
  int32_t nxy, nth;                    /* the lattice: (2 nxy + 1)^2 (2 nth + 1) candidates */
  double step_xy, step_th;
  const double *rot;                   /* [2 nth + 1][2] */
  double *pose_out;                    /* [B][3] out */
  int32_t *best, *score;               /* [B] out */
  int32_t *score0, *used;              /* [B] out, may be NULL */
} rmpc_scan_match;
int rmpc_grid_edge_distance_device(int H, int W, const double *d_grid, double occ_threshold, int sub, int cap,
                                   int32_t *d_d2, void *stream);
int rmpc_lidar_project_device(int B, const rmpc_lidar *l, void *stream);
int rmpc_scan_match_device(int B, const rmpc_scan_match *m, void *stream);

/* Wide-window localisation: the pose of rmpc_scan_match_device over a lattice of up to 255 x 255 x 255,
 * found by branch and bound (Olson 2009, the multi-resolution half) instead of by scoring every candidate.  Needs no
 * handle; every pointer is a device pointer, each call runs on the device of its first pointer (d_d2, s->pose), takes
 * a stream and never synchronises.  Bounds are int32 sums of table entries that no candidate below a node undercuts,
 * so the result is the exhaustive rule's bit for bit, on every run and whatever the order of the search.
 *
 * rmpc_grid_min_pyramid_device: from d_d2 [FH][FW] (FH = H sub, FW = W sub; the table of
 * rmpc_grid_edge_distance_device) d_pyr [levels][FH][FW] int32, level major: pyr [l][R][C] = the least d2 over the
 * window [R, R + 2^l) x [C, C + 2^l) intersected with the map; level 0 is d2 itself.  One launch per level.  Refused:
 * NULL pointers, H or W < 1, H W > RMPC_GRID_MAX_CELLS, sub outside [1, 8], levels outside [1, 12].
 *
 * rmpc_scan_search_device: rules 1 to 5 of rmpc_scan_match_device over the lattice nxy, nth <= RMPC_SEARCH_MAX_N, with
 * the same used rays, the same expressions for qx, qy, C, R in the same order, the same cap outside the map and the
 * same order (score, m, k), compared as the tuple (k < 2^24 and m < 2^16 no longer fit one word beside a 31-bit
 * score); pose_out, best, score, score0 (always the centre candidate's exact score) and used are those of that rule.
 * A robot with active [b] == 0 (active may be NULL: every robot is active) gets rule 1's outputs, pose_out = the
 * prior, best -1, score = score0 = 0, and used = its count of used rays.  rot comes from the caller as before.
 *
 * The bound.  A node is one rotation jth and a block of translations jx in [a, a1], jy in [b, b1], a and b multiples
 * of 2^h and a1 = min(a + 2^h, 2 nxy + 1) - 1 (b1 likewise), h = top_log2 at the top level, one less per level and 0 at
 * a leaf, which is one candidate and is scored by rule 4.  Of a node with h > 0, per used ray, with rule 4's
 * expressions as doubles: Ca, Cb = the fine columns at jx = a and jx = a1, Ra, Rb = the fine rows at jy = b and
 * jy = b1.  Any of the four not finite: the term is 0.  Else Cb < 0 or Ca >= FW or Rb < 0 or Ra >= FH: the term is
 * cap.  Else all four are clipped into the map, e = max(Cb - Ca, Rb - Ra) + 1, l = the least level with 2^l >= e, and
 * the term is pyr [l][Ra][Ca], or 0 when l >= levels.  The bound is the int32 sum of the terms; the node's key is
 * (bound, m_min, 0) with m_min the least m of its block, and a node is dropped only when its key is greater than the
 * full key (score, m, k) of the best candidate scored so far.
 *
 * The top-level nodes are numbered t = (jth nb + b / 2^top_log2) nb + a / 2^top_log2, nb = ceil((2 nxy + 1) / 2^top_log2),
 * ntop = (2 nth + 1) nb nb.  top_bound [B][ntop] (may be NULL) receives their bounds, of the robots that were searched
 * only: the rows of the others are not written.  leaves [B] (may be NULL) = the number of candidates scored exactly, a
 * diagnostic that may depend on the schedule (0 for a robot that was not searched; the centre candidate's extra
 * scoring for score0 is not counted).  work holds the bound table when top_bound is NULL: the kernel writes at most
 * 4 B ntop bytes of it, rmpc_scan_search_work_bytes (B, nxy, nth, top_log2) says how many (-1 on arguments out of
 * range); the nodes being searched live in a store of fixed size on the chip that cannot overflow.
 * struct_size must equal sizeof(rmpc_scan_search); refused (-1, rmpc_last_error) as by rmpc_scan_match_device, with
 * nxy or nth outside [0, RMPC_SEARCH_MAX_N], and: top_log2 outside [0, 7], levels outside [1, 12], a NULL pyr or work,
 * work_bytes below the query's value, B ntop beyond INT_MAX. */
#define RMPC_SEARCH_MAX_N 127
typedef struct rmpc_scan_search {
  int32_t struct_size;                 /* sizeof(rmpc_scan_search) */
  int32_t rays;                        /* R in [1, RMPC_MATCH_MAX_RAYS] */
  const double *pose;                  /* [B][pose_stride]: the priors, x, y, heading at 0, 1, 2 */
  const double *points;                /* [B][R][3]: the scan projected at the priors */
  const double *ranges;                /* [B][R] */
  double range;                        /* the scan's range (> 0): t < range is a hit */
  int32_t pose_stride, min_hits;       /* >= 3; >= 1 */
  const int32_t *d2;                   /* [H sub][W sub] */
  int32_t H, W, sub, cap;
  double x0, y0, cell;
  int32_t nxy, nth;                    /* the lattice: (2 nxy + 1)^2 (2 nth + 1) candidates, each n <= 127 */
  double step_xy, step_th;
  const double *rot;                   /* [2 nth + 1][2] */
  double *pose_out;                    /* [B][3] out */
  int32_t *best, *score;               /* [B] out */
  int32_t *score0, *used;              /* [B] out, may be NULL */
  const int32_t *pyr;                  /* [levels][H sub][W sub]: rmpc_grid_min_pyramid_device of d2 */
  int32_t levels, top_log2;            /* [1, 12]; [0, 7] */
  const int32_t *active;               /* [B], may be NULL: 0 = leave this robot at its prior */
  void *work;                          /* work_bytes >= rmpc_scan_search_work_bytes(B, nxy, nth, top_log2) */
  int64_t work_bytes;
  int32_t *leaves;                     /* [B] out, may be NULL */
  int32_t *top_bound;                  /* [B][ntop] out, may be NULL */
} rmpc_scan_search;
int rmpc_grid_min_pyramid_device(int H, int W, int sub, const int32_t *d_d2, int levels, int32_t *d_pyr, void *stream);
int64_t rmpc_scan_search_work_bytes(int B, int nxy, int nth, int top_log2);
int rmpc_scan_search_device(int B, const rmpc_scan_search *s, void *stream);

/* Moving obstacles: a multi-target tracker per robot, from one lidar scan to the obst_dyn array a scene
 * points at (rmpc_scene.obst_dyn, predicted by the solver per stage at dt k).  Needs no handle; every pointer is a
 * device pointer, the call runs on the device of its first pointer (points), takes a stream and never synchronises.  The
 * chain per control step is
 *   rmpc_lidar_scan_device (or rmpc_lidar_project_device) -> [rmpc_lidar_scan_device of the static world alone]
 *   -> rmpc_plan_points_device (d_z_prev = NULL, N = 1: the sensor origins) -> rmpc_lidar_tracks_device.
 * The kernel evaluates + - * / sqrt on doubles in the order written (no sin / cos, no contraction) and every choice is
 * a minimum under a strict total order: every result is bitwise the same on every run and equals the numpy restatement
 * (tests/tracking_reference.py).  The rules are the project's own.  Per robot b with p_i = points [b][i][0 .. 1],
 * t_i = ranges [b][i], o = origin [b][0 .. 1], R = rays, T = n_tracks:
 *  1. ray i is MOVING iff t_i < static_ranges [b][i] - margin, or, when static_ranges is NULL, iff t_i < range (a NaN
 *     compares false);
 *  2. the predecessor of ray i is i - 1, of ray 0 it is R - 1 when closed != 0 (a full sweep) and none otherwise; it
 *     LINKS when it is moving and (dx dx + dy dy) <= gap gap, d = p_i - p_pred.  Ray i STARTS a segment iff it is moving
 *     and its predecessor does not link; a closed sweep whose rays are all moving and none of which starts takes ray 0
 *     as its start.  A segment runs from its start to the ray before the next start or the next ray that is not
 *     moving, around the seam when closed.  Segments are ordered by start ray; counts [b][0] = their number.  A segment
 *     is dropped when it has fewer than min_rays rays, or when max_extent > 0 and the squared distance from its first
 *     to its last point exceeds max_extent max_extent; the first RMPC_TRACK_MAX_DET that remain are the detections,
 *     counts [b][1] = their number;
 *  3. a detection's centre, the circle of the known radius through its n points: m = (the sum of the points in segment
 *     order) / n; w = m - o, c = m + radius (w / sqrt(wx wx + wy wy)); then four times: per point q = p_i - c,
 *     r = sqrt(qx qx + qy qy), u = q / r, e = r - radius, the sums a11 += ux ux, a12 += ux uy, a22 += uy uy, gx += ux e,
 *     gy += uy e in segment order from 0; a11 += 1e-3, a22 += 1e-3, D = a11 a22 - a12 a12,
 *     cx += (a22 gx - a12 gy) / D, cy += (a11 gy - a12 gx) / D.  No case split for n = 1 or 2.  det [b][k] = the centre
 *     z_k of detection k, (0, 0) in the unused rows;
 *  4. slot j is LIVE iff age [b][j] > 0.  Predict: pred_j = p_j + v_j dt.  Associate: the pairs (live j, k) with
 *     s = (dx dx + dy dy) <= gate gate, d = pred_j - z_k, are visited in ascending (s, j, k) and a pair is taken when
 *     neither side has been.  A matched track: res = z - pred, p = pred + alpha res, v = v + (beta res) / dt, each
 *     component of v then limited to [-v_max, v_max] when v_max > 0; age + 1 (held at INT32_MAX), miss = 0.  An
 *     unmatched live track coasts: p = pred, miss + 1 (held at INT32_MAX), and age = 0 (the slot is free, its other
 *     words stay) when miss > max_miss.  Births: the unmatched detections in their order take the lowest free slots,
 *     those freed in this call included, with p = z, v = 0, age = 1, miss = 0; detections that find none are lost;
 *  5. the CONFIRMED tracks (age >= confirm) ordered by ((dx dx + dy dy), j), d = p_j - o (a NaN distance counts as
 *     +inf): the first n_out become obst_dyn [b][row] = (px, py, 0, vx, vy, 0, 0, 0, 0), every further row is
 *     (park_x, park_y, 0, 0, 0, 0, 0, 0, 0).  counts [b][2] = the live tracks, counts [b][3] = the confirmed ones, both
 *     after the call.
 * track, age and miss are the filter's state, zero-filled by the caller before the first call and carried between
 * calls.  A robot's rows are written by its own workgroup alone; there are no atomics on memory.
 * struct_size must equal sizeof(rmpc_tracks); refused (-1, rmpc_last_error) before any device call: NULL pointers other
 * than static_ranges, det and counts, B < 1, rays outside [1, RMPC_TRACK_MAX_RAYS], n_tracks outside
 * [1, RMPC_TRACK_MAX_TRACKS], n_out < 1, min_rays < 1, confirm < 1, max_miss < 0, a range, gap, radius, gate or dt that
 * is not positive and finite, alpha outside (0, 1], beta outside [0, 2], a margin, max_extent or v_max that is negative
 * (or NaN), park_x or park_y not finite, obst_dyn overlapping track, and B rays 3, B n_tracks 4 or B n_out 9 beyond
 * INT_MAX. */
#define RMPC_TRACK_MAX_RAYS 2048
#define RMPC_TRACK_MAX_TRACKS 16
#define RMPC_TRACK_MAX_DET 16
typedef struct rmpc_tracks {
  int32_t struct_size;                 /* sizeof(rmpc_tracks) */
  int32_t rays;                        /* R in [1, RMPC_TRACK_MAX_RAYS] */
  int32_t closed, min_rays;            /* != 0: rays R - 1 and 0 are neighbours; >= 1 */
  const double *points;                /* [B][R][3]: the scan */
  const double *ranges;                /* [B][R] */
  const double *static_ranges;         /* [B][R]: the scan of the known static world at the same pose, may be NULL */
  const double *origin;                /* [B][3]: the sensor origins */
  double range, margin, gap, radius, max_extent;
  double gate, dt, alpha, beta, v_max;
  double park_x, park_y;
  int32_t confirm, max_miss;           /* >= 1; >= 0 */
  int32_t n_tracks, n_out;             /* T in [1, RMPC_TRACK_MAX_TRACKS]; >= 1 */
  double *track;                       /* [B][T][4] in/out: px, py, vx, vy */
  int32_t *age, *miss;                 /* [B][T] in/out; age 0 = a free slot */
  double *obst_dyn;                    /* [B][n_out][9] out */
  double *det;                         /* [B][RMPC_TRACK_MAX_DET][2] out, may be NULL */
  int32_t *counts;                     /* [B][4] out, may be NULL: segments, detections, live, confirmed */
} rmpc_tracks;
int rmpc_lidar_tracks_device(int B, const rmpc_tracks *t, void *stream);

/* Timed routes: conflict-free space-time routes for a fleet, decided before anyone moves, and the
 * follower that keeps their order.  Needs no handle; every pointer is a device pointer, each call runs on the device of
 * its first pointer (grid, d_paths), takes a stream and never synchronises.  Everything is integer work on cells except
 * the ranking of end cells, which compares the doubles of a field as written: every result is bitwise the same on every
 * run.  Cell c = row * W + col; d2(c, c') = (r - r')^2 + (col - col')^2; two cells CONFLICT when d2 < sep2.
 *
 * rmpc_timed_plan_device: prioritised planning (cooperative A*, Silver 2005) of B robots over the window t = 0 .. T, for
 * G priority orders at once.  grid [H][W] with the class data >= occ_threshold occupied (a NaN is free); movement 4 or
 * 8: the planner's first `movement` moves m = (dcol, drow) in its own order; start_cell [B]; goal_index [B] into
 * fields [Gf][H][W], the output of rmpc_grid_fields_device for goal_cells [Gf] on this grid (read only to rank end
 * cells and to tell arrival; they must hold no NaN); orders [G][B] int32, each row a permutation of 0 .. B - 1, rank 0
 * planned first.  Order g takes its robots in rank order; res[t] (t = 0 .. T) starts empty:
 *  1. robot b is SKIPPED when start_cell [b] lies outside [0, H W) or goal_index [b] outside [0, Gf): status
 *     RMPC_GRID_OUTSIDE, path all -1, arrive T + 1; it stamps nothing and blocks nobody;
 *  2. reach[0] = {start}: the start is exempt from every test (a robot stands where it stands, as in
 *     rmpc_grid_descend_device);
 *  3. for t = 1 .. T, reach[t] holds c when c is free on the grid, res[t] does not hold c, for t <= lag c does not
 *     conflict with the start of a later-ranked robot that is not skipped, and reach[t - 1] holds c (a wait) or c - m
 *     for a move m with c - m inside the map (a diagonal move needs only its end cell free, as in the reference's A*);
 *  4. if reach[f] is empty for a least f >= 1 the robot FAILS: status = f, te = f - 1; otherwise status = 0, te = T;
 *  5. the end cell is the c of reach[te] that is least by (D(c), c), D = fields [goal_index [b]]; a D that is not below
 *     +inf ranks as +inf, ties go to the lower cell;
 *  6. p[te .. T] = the end cell; backwards from te, the predecessor of (t, c) is c itself when reach[t - 1] holds c (wait
 *     first), otherwise c - m for the first move m in move order with c - m inside the map and in reach[t - 1].  Waiting
 *     first at the end cell makes the arrival the earliest that can be held until T;
 *  7. arrive [b] = the least a with p[a .. T] all equal to goal_cells [goal_index [b]], T + 1 when there is none;
 *  8. for every t, the cells that conflict with p[t] are set in res[s] for every s in [0, T] with |s - t| <= lag.  A
 *     failed robot stamps too, so that later ranks avoid it.
 * Outputs: paths [G][B][T + 1], status [G][B], arrive [G][B] int32; key [G] int64 = (fails << 44) | (late << 32) |
 * sum_arrive with fails the robots of status > 0, late those with arrive > T (skipped ones too), sum_arrive the sum of
 * arrive (a late robot adds T + 1): the limits below keep every part inside its bits; best: one int32, the g with the
 * least (key, g) among the rows that are permutations.  A row that is not a permutation gets RMPC_TIMED_BAD_ORDER in
 * every status, -1 in every path cell, arrive T + 1 and the key INT64_MAX; best = -1 when no row is valid.
 * GUARANTEE: between two robots i, j of one order that both have status 0, d2(p_i[t], p_j[s]) >= sep2 whenever
 * |s - t| <= lag, by construction: the later-ranked of the two reached every p[t], t >= 1, through res[t], which holds
 * the earlier one's stamps of all s within lag of t; at t = 0 it stands on its start, which the earlier one avoided
 * during its first `lag` layers and which differs from the earlier one's start by the caller's choice (starts closer
 * than sep2 are planned all the same: the exemption).  Vertex, swap and following conflicts are instances of it.
 * work: a workspace of rmpc_timed_plan_work_bytes(H, W, T, G) bytes (work_bytes: its size), contents irrelevant.
 * struct_size must equal sizeof(rmpc_timed_plan); refused (-1, rmpc_last_error): NULL pointers, H or W < 1,
 * H W > RMPC_GRID_MAX_CELLS, a movement other than 4 or 8, B outside [1, RMPC_TIMED_MAX_ROBOTS], T outside
 * [1, RMPC_TIMED_MAX_T], G outside [1, RMPC_TIMED_MAX_ORDERS], sep2 outside [1, RMPC_TIMED_MAX_SEP2], lag outside
 * [1, RMPC_TIMED_MAX_LAG], Gf < 1, Gf H W or G B (T + 1) beyond INT_MAX, a workspace that is too small.
 * rmpc_timed_plan_work_bytes returns -1 for sizes the plan refuses.
 *
 * rmpc_timed_follow_device: rmpc_follow_path_device for one order's d_paths [B][T + 1], one simultaneous step of all
 * robots: d_idx_out [B] is a different buffer from d_idx_in [B] (refused otherwise), so the result does not depend on
 * the order in which the device's lanes meet.  With i = d_idx_in [b] clamped to [0, T], robot b advances to i + 1 when
 *  - i < T and the distance from d_pos [b * stride + 0 .. 1] to the centre of p_b[i] is <= threshold, and
 *  - for every j != b whose path is valid and every s <= i - lag with d2(p_j[s], p_b[i + 1]) < sep2:
 *    d_idx_in [j] >= s + lag (j has left the layers whose stamps b's next cell was planned around).
 * d_blocked [b] (may be NULL) = the lowest j that fails the second test, -1 when none does or the first test fails.
 * Then d_goal [b] = (centre of p_b[d_idx_out [b]], 0).  A robot whose path starts with -1 keeps its goal and its index
 * (d_idx_out [b] = d_idx_in [b], d_blocked [b] = -1) and blocks nobody.
 * LIVENESS: among robots that are all at their waypoints and not all at T, take one whose pending layer t = idx + 1 is
 * least: every idx_j >= t - 1, and every blocking s has s + lag <= idx = t - 1 <= idx_j, so it is not blocked.  The
 * plan's order is kept and cannot deadlock: a robot that runs late delays the others and does not meet them.
 * Refused: NULL pointers other than d_blocked, d_idx_out == d_idx_in, B, T, sep2 or lag outside the plan's limits,
 * stride < 2, W < 1, B stride beyond INT_MAX. */
#define RMPC_TIMED_MAX_ROBOTS 1024
#define RMPC_TIMED_MAX_T 1023
#define RMPC_TIMED_MAX_ORDERS 1024
#define RMPC_TIMED_MAX_SEP2 4096
#define RMPC_TIMED_MAX_LAG 4
#define RMPC_TIMED_BAD_ORDER (-8)       /* the row of orders is not a permutation of 0 .. B - 1 */
typedef struct rmpc_timed_plan {
  int32_t struct_size;                 /* sizeof(rmpc_timed_plan) */
  int32_t H, W, movement;
  const double *grid;                  /* [H][W] */
  double occ_threshold;
  int32_t B, Gf;
  const int32_t *start_cell;           /* [B] */
  const int32_t *goal_index;           /* [B] into fields / goal_cells */
  const double *fields;                /* [Gf][H][W] */
  const int32_t *goal_cells;           /* [Gf] */
  int32_t T, sep2, lag, G;
  const int32_t *orders;               /* [G][B] */
  void *work; int64_t work_bytes;
  int32_t *paths, *status, *arrive;    /* [G][B][T + 1], [G][B], [G][B] out */
  int64_t *key;                        /* [G] out */
  int32_t *best;                       /* one int32 out */
} rmpc_timed_plan;
int64_t rmpc_timed_plan_work_bytes(int H, int W, int T, int G);
int rmpc_timed_plan_device(const rmpc_timed_plan *p, void *stream);
int rmpc_timed_follow_device(int B, int T, const int32_t *d_paths, const int32_t *d_idx_in, int32_t *d_idx_out,
                             const double *d_pos, int stride, int W, double x0, double y0, double cell, double threshold,
                             int sep2, int lag, double *d_goal, int32_t *d_blocked, void *stream);

/* Fleet separation: a separating plane per neighbour pair and stage, in the style of buffered Voronoi
 * cells, written into the lin_constrs slots of an rmpc_scene: the LinearConstraints row |a.p + d| / |a| - r_body >= 0
 * keeps the collision link clear of each.
 * Needs no handle; every pointer is a device pointer, each call runs on the device of its first pointer.
 * rmpc_fleet_points_device: the predicted collision points d_points [B][N][3] of the coming solve.  Stage k reads
 * q = d_z_prev [b][min(k + 1, N - 1)][0 .. 2] (the previous plan shifted by the applied u_0, its last stage held), or
 * q = d_pose [b * pose_stride + 0 .. 2] when d_z_prev is NULL or d_exitflag [b] < 0 (d_exitflag may be NULL).
 * heading = 1 (the boxer): the point is (x + offset_x cos q2 - offset_y sin q2, y + offset_x sin q2 + offset_y cos q2,
 * height) as in rmpc_plan_points_device; heading = 0 (the point robot): (q0, q1, height).  Refused: NULL d_pose or
 * d_points, B < 1, N < 1, heading other than 0 or 1, pose_stride < 3, nvar < 3, and B*N, B*pose_stride or B*N*nvar
 * beyond INT_MAX.
 * rmpc_fleet_planes_device: for robot b at stage k, q_j = d_points [j][k] and s_j = |q_j - q_b|^2, the candidates are
 * the robots j != b with s_j < range^2 (range = 0 admits nobody, +inf everyone); the K of least s_j (ties to the lower
 * j) write slots slot0 .. slot0 + K - 1 of d_planes [B][N][nobst][4].  With lo = min(b, j), hi = max(b, j):
 * u = q_lo - q_hi, d = |u|, n = u / d ((1, 0, 0) when d = 0), g = d - r_lo - r_hi, m = q_hi + (r_hi + g / 2) n,
 * c = -n.m; robot lo gets (n, c), robot hi (-n, -c), so both predicted points lie r_own + g / 2 from the plane.  Slots
 * without a candidate get the dummy plane of rmpc_free_space_device around q_b; the other slots are left untouched.
 * d_radius [B] = r_body.  Refused: NULL pointers, B < 1, N < 1, K < 1, K > 8, slot0 < 0, slot0 + K > nobst, a
 * negative or NaN range, and B*N*nobst*4 beyond INT_MAX. */
int rmpc_fleet_points_device(int B, int N, const double *d_z_prev, int nvar, const int32_t *d_exitflag,
                             const double *d_pose, int pose_stride, int heading, double offset_x, double offset_y,
                             double height, double *d_points, void *stream);
int rmpc_fleet_planes_device(int B, int N, const double *d_points, const double *d_radius, int K, double range,
                             int nobst, int slot0, double *d_planes, void *stream);

/* Debug / parity hooks (used by tests through the same ABI): evaluate one
 * stage-parallel sweep at z = x0 (first-pass semantics) and return the
 * condensed stage blocks in instance-major order.
 * out_Q [B][N][nvar*nvar] dense symmetric, out_q0/out_q1 [B][N][nvar],
 * out_rc [B][N][nx], out_g [B][N][nh], out_f [B][N]. */
int rmpc_debug_sweep(rmpc_handle *h, int B, const double *xinit, const double *x0,
                     const double *params, double *out_Q, double *out_q0,
                     double *out_q1, double *out_rc, double *out_g, double *out_f);

/* Debug / parity hook (tests only): ONE first sweep and ONE Riccati recursion of B instances on the path this handle
 * runs in production -- the pass kernels (k_sweep, then k_riccati / k_riccati_lane as the batch size and the
 * development switches select them) or, on a fused handle, the phase functions of k_fused / k_fused_arm -- and the
 * Newton step that came out.  lam_w [B][N][m], nu_w [B][N][nx], mu_w [B]: multipliers, costates and final barrier
 * parameter of a previous solve as a warm-started handle stores them (stage k starts from the values of stage k + 1);
 * all three NULL: the cold first pass.  The recursion runs on the Gauss-Newton blocks (no curvature terms), so that
 * the returned blocks are what it consumed.  Instance-major outputs: out_Q [B][N][nvar*nvar], out_q0 / out_q1
 * [B][N][nvar] (q = q0 - mu q1), out_rc [B][N][nx] as rmpc_debug_sweep; out_t / out_lam [B][N][m] slacks and
 * multipliers the blocks were built with, out_mu [B]; out_dz [B][N][nvar] the step, out_nu [B][N][nx] the new
 * costates (stage 0, the multiplier of the fixed first state, is formed by no path and read by nothing: zeros),
 * out_ok [B] the recursion's return value (1: every control block was positive definite).  Forgets the
 * stored multipliers of a warm-started handle.  m_rows: the m the caller sized out_t / out_lam
 * for (refused when it is not the model's).  out_path [4] (may be NULL): what the handle holds of the switches that
 * select the path -- fused kernel (0 none, 1 k_fused, 2 k_fused_arm), the lane-per-instance setting (RMPC_RIC_LANE:
 * 0 never, 1 large lists, 2 always), parts per stage of k_fused_arm (0: not that kernel), 1 when a generated view runs. */
int rmpc_debug_step(rmpc_handle *h, int B, const double *xinit, const double *x0, const double *params,
                    const double *lam_w, const double *nu_w, const double *mu_w, double *out_Q, double *out_q0,
                    double *out_q1, double *out_rc, double *out_t, double *out_lam, double *out_mu, double *out_dz,
                    double *out_nu, int32_t *out_ok, int m_rows, int32_t *out_path);

/* rmpc_debug_step with the curvature terms (tests only).  The sweep runs with the model's own curvature setting (the
 * exact second-order terms of the distance rows and the inverse-barrier objective, the arms' second derivatives of the
 * kinematics, the unicycle's frame rotation and nu . grad^2 Phi of its dynamics with the costates of the first pass) and
 * the recursion on  H = out_Q - cw out_C:  out_Q the Gauss-Newton blocks as above, out_C [B][N][nvar*nvar] (may be NULL)
 * the dense symmetric matrix the recursion subtracts per unit weight, unpacked from the stage records by the host: the
 * q block, and for the unicycle the entries over (theta, omega, u1 | v, u0); zero where the model has no terms (all of
 * it for a model that uses none, e.g. a holonomic chain with the slack variable).  cw in [0, 1]: 1 the exact Hessian,
 * 1/2, 1/4 the scaled curvature of the small holonomic chains, 0 Gauss-Newton; k_fused_arm takes 0 or 1 only.  The
 * pass kernels: k_riccati's recursion is called at cw as the fused kernels' is; k_riccati_lane decides its weight from
 * the instance (the barrier parameter at or below 1e-2: the instance's scale, set to cw here; else 0) and the call
 * fails when the first pass cannot run at cw.  out_ok: 0 where a control block was not positive definite (the return
 * value that drives the Gauss-Newton fallback, the back-off and the half-weight retry); out_dz / out_nu are then
 * unspecified.  cw = 0 and out_C = NULL is rmpc_debug_step, bit for bit. */
int rmpc_debug_step_curv(rmpc_handle *h, int B, const double *xinit, const double *x0, const double *params,
                         const double *lam_w, const double *nu_w, const double *mu_w, double *out_Q, double *out_q0,
                         double *out_q1, double *out_rc, double *out_t, double *out_lam, double *out_mu, double *out_dz,
                         double *out_nu, int32_t *out_ok, int m_rows, int32_t *out_path, double cw, double *out_C);

/* Generated solvers.  The reference has FORCES Pro generate C code for ONE problem (mpcModel.py:139-160
 * generateSolver, examples/makeSolver.py); here the kernels exist in two forms: over runtime row tables (any
 * descriptor) and over "generated views" -- the same tables as compile-time constants, so that the row loops of
 * the hot kernels become straight-line code (csrc/rmpc_spec_gen.hpp: views of the point-robot configurations).
 * rmpc_spec_source writes the C++ text of the view of `desc` (struct `name`) into out (cap bytes incl. the
 * terminating 0) and returns the size it needs, or -1; scripts/gen_specs.py assembles the header from it.
 * rmpc_create selects a view when every table entry equals the descriptor's (RMPC_NO_SPEC=1 in the environment
 * forces the runtime tables; measured: same throughput, one batch alone 6 % faster on the point robot, 20 % slower
 * on the boxer, whose views are therefore not generated: DESIGN.md 5.1); rmpc_spec_name returns the view's name
 * ("" = runtime tables). */
int64_t rmpc_spec_source(const rmpc_desc *desc, const char *name, char *out, int64_t cap);
const char *rmpc_spec_name(rmpc_handle *h);
const char *rmpc_spec_for(const rmpc_desc *desc);   /* the view rmpc_create would select (no GPU needed) */

/* Test aid: overwrites the LDS of every CU of the handle's device with NaN patterns (tests/test_gpu_parity.py:
 * a solve must not depend on what a previous kernel left in LDS). */
int rmpc_debug_poison_lds(rmpc_handle *h);

/* Test aid: which kernels the host loop enqueued for the last solve of this handle, so that a test of a batch regime can
 * assert that it ran in it.  Host only: filled in as the solve is enqueued, no device read, no synchronisation.
 *   out[0]  passes enqueued when the survivors moved to the compact workspace (k_migrate), -1: they did not
 *   out[1]  survivors moved, -1: none
 *   out[2]  recursion kernel of the first pass, RMPC_PATH_RIC_*
 *   out[3]  recursion kernel of the last pass enqueued.  k_riccati's grouped and one-wave blocks are both launched
 *           for a list of at least 512 columns and the list's length on the device picks one: GROUPED is reported
 *           until a look of the host loop has found that length below 512 (it never grows), WAVE from then on; a
 *           solve under a pass budget takes no looks and reports what it launched
 *   out[4]  list builder run on the whole batch, RMPC_PATH_COMPACT_* (after a migration the survivors' list is built
 *           by k_compact_wave whatever the batch)
 *   out[5]  1: the solve was one fused launch, out[0 .. 4] are -1
 * Before the first solve out[0 .. 4] are -1. */
#define RMPC_PATH_RIC_WAVE 0      /* k_riccati<C, 1>: one wavefront per instance */
#define RMPC_PATH_RIC_GROUPED 1   /* k_riccati<C, IPB>: several instances per block, half a wavefront each for small models */
#define RMPC_PATH_RIC_LANE 2      /* k_riccati_lane: one lane per instance */
#define RMPC_PATH_COMPACT_WAVE 0  /* k_compact_wave */
#define RMPC_PATH_COMPACT_BLOCK 1 /* k_compact */
int rmpc_last_solve_path(const rmpc_handle *h, int32_t out[6]);

/* Test aid: the whole-horizon reductions of the kernels (sums, maxima, minima over the lpi = 32 or 64 consecutive lanes of
 * an instance) run by one wavefront on device `device` over caller-supplied lane values, once with the shuffle exchanges
 * (the reference form) and once with the vector-move exchanges the kernels use.  in, out_shfl, out_dpp: [10][64] doubles,
 * word w of lane l at [w][l].  op 0 / 1 / 2: sum / maximum / minimum of word 0; op 3: the sweep's partials together, sums
 * of words 0 .. 4, maxima of 5 .. 8, minimum of 9; op 4: the step lengths together, the sum of word 0 and the minima of
 * words 1 and 2 (word 3 of the outputs: the maximum of the constant zero the kernels pass along).  Every lane's result
 * is returned; words an op does not use come back as zeros. */
int rmpc_debug_wave_reduce(int device, int lpi, int op, const double *in, double *out_shfl, double *out_dpp);

/* Development aid: per-block phase cycle counts of the last fused launch (8 words per block: sweep, decisions,
 * recursion, step, total, passes, start, -); all zero unless the library was built with -DRMPC_STAMPS. */
int rmpc_debug_fused_stamps(rmpc_handle *h, long long *out, int nblocks);

#ifdef __cplusplus
}
#endif
#endif
