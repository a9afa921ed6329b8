// rmpc_host.hpp -- what the host unit (rmpc_host.hip) and the variant units (rmpc_variants.hip) share: the handle,
// the error channel (rmpc_err.hpp) and the table through which the host reaches the kernels of a variant.
#pragma once
#include "rmpc_kernels.hip"
#include "rmpc_err.hpp"

using namespace rmpc;

enum KernelId { K_PACK = 0, K_SWEEP, K_RICCATI, K_STEP, K_UNPACK, K_FUSED };

struct VariantOps;

struct rmpc_handle {
  rmpc_desc desc;
  DevModel M;
  DevTables T;
  DevTables *d_T = nullptr;
  Ws W;
  Ws Wc;            // compact workspace the last survivors of a batch migrate to (Bpc columns; Bpc == 0: none)
  int Bpc = 0;
  int warm_mode = 0;        // rmpc_set_warm_start
  bool have_duals = false;  // the warm-start arrays hold the multipliers of a finished solve of duals_B instances
  int duals_B = 0;
  const VariantOps *ops = nullptr;   // kernel variant and view this handle runs (rmpc_create)
  bool fused = false;   // this model runs the fused kernel (small models, N <= 32); the pass kernels otherwise
  int ric_lane = 1;       // lane-per-instance recursion of the pass kernels: 0 never, 1 large lists, 2 always (RMPC_RIC_LANE)
  int fused_grid = 1024;  // wavefronts the chip holds at one per SIMD (4 x compute units): grid of a fused launch
  FusedWs F;
  int *h_passes = nullptr;  // pinned
  int device = 0;
  int max_batch = 0;
  int Bp = 0;
  int max_passes = 0;
  int pass_budget = 0;            // rmpc_set_pass_budget (0: none)
  int packed_B = 0;               // batch size of the parameters rmpc_pack_scene_workspace left in the workspace
  void *ws_base = nullptr;
  size_t ws_bytes = 0;
  hipStream_t stream = nullptr;
  // staging for the host-pointer entry point
  double *d_xinit = nullptr, *d_x0 = nullptr, *d_params = nullptr, *d_zout = nullptr, *d_kkt = nullptr,
         *d_obj = nullptr;
  int *d_exit = nullptr, *d_iters = nullptr;
  int *h_active = nullptr;  // pinned
  int last_passes = 0;
  int last_cap = 0;             // passes enqueued by the last solve of the pass kernels
  // rmpc_last_solve_path (test aid): what solve_device enqueued for the last solve, kept on the host as it enqueues
  int ric_sel = -1;             // recursion launch_pass selected last (RMPC_PATH_RIC_*; grouped: both launched, the list decides)
  int path[6] = {-1, -1, -1, -1, -1, 0};
  // profiling
  bool profiling = false;
  std::vector<hipEvent_t> ev;   // pool, reused across solves
  size_t ev_used = 0;
  std::vector<int> ev_kind;
  double prof_ms[RMPC_NUM_KERNELS] = {0};
  int64_t prof_n[RMPC_NUM_KERNELS] = {0};
  int64_t lane_bytes[RMPC_NUM_KERNELS] = {0};   // per active lane (pack/unpack: per call)
  double prof_bytes[RMPC_NUM_KERNELS] = {0};     // accumulated algorithmic bytes of the profiled launches
  std::vector<int> h_hist;
  // debugging switches, read once at rmpc_create (never set by the product code)
  bool env_no_migrate = false, env_no_order = false, env_no_cold_order = false, env_arm_two_parts = false;
};

// The workspace the passes currently run in: the batch's own, or the compact one after migration
// (B = number of columns in use).
struct Phase {
  Ws W;
  int B;
};

// Host view of the stage-record layout, for the host code that sizes or reads records without a variant at hand
// (rmpc_workspace_bytes, rmpc_debug_sweep).  rmpc_variants.hip checks it against Cfg::R_* of every variant it builds.
struct RecLayout { int q, c, dg, cs, q0, q1, rc, a5, b5, d, rw, rs; };
constexpr RecLayout rec_layout(int robot, int n, int nv, int ns, int nx) {
  RecLayout L{};
  const int nq2 = n * (n + 1) / 2;
  L.q = 0; L.c = nq2; L.dg = 2 * nq2; L.cs = L.dg + (nv - n);
  L.q0 = L.cs + (ns > 0 ? nv : 0); L.q1 = L.q0 + nv; L.rc = L.q1 + nv;
  L.a5 = L.rc + nx; L.b5 = L.a5 + 25; L.d = L.b5 + 10;
  L.rw = L.a5 + (robot == RMPC_ROBOT_DIFFDRIVE ? 35 + 11 : 0);   // (+ Cfg::ND curvature entries)
  L.rs = (L.rw + 1 + 7) / 8 * 8;
  return L;
}
inline RecLayout rec_layout(const DevModel &M) { return rec_layout(M.robot, M.n, M.nv, M.ns, M.nx); }

// One entry per (kernel variant, view) the library holds: the variant's runtime-table view and each generated view
// of rmpc_spec_gen.hpp with the variant's robot and size.  The unit that builds a variant adds its entries while the
// library loads (rmpc_variants.hip); a handle picks one at rmpc_create and reaches every kernel of its variant through it.
struct VariantOps {
  int robot, nq, ns;   // Cfg::ROBOT, NQ, NS
  const char *spec;    // name of the generated view, "" for the runtime tables
  bool (*matches)(const rmpc_desc &, const DevModel &, const DevTables &);   // generated view: equals these tables
  bool fused;          // Cfg::FUSED_OK || Cfg::ARM_FUSED: a fused kernel exists
  bool arm_fused;      // Cfg::ARM_FUSED: it is k_fused_arm
  int rs;              // Cfg::RS: stage-record stride
  // pass kernels: k_sweep, k_riccati[_lane] or k_step (which = K_SWEEP / K_RICCATI / K_STEP)
  void (*pass)(rmpc_handle *h, const Phase &ph, int first, int pass, hipStream_t st, int which);
  // k_difficulty (cold launch order of k_fused), nullptr: none
  void (*difficulty)(rmpc_handle *h, int B, const double *d_xinit, const double *d_params, hipStream_t st);
  // k_fused / k_fused_arm, nullptr: none
  void (*fused_launch)(rmpc_handle *h, int B, const double *d_xinit, const double *d_x0, const double *d_params,
                       double *d_zout, int *d_exit, int *d_iters, double *d_kkt, double *d_obj, hipStream_t st, int cap,
                       int warm, int use_order);
  // test aid (rmpc_debug_step[_curv], rmpc_step_debug.hpp): first sweep and recursion of the fused kernel, nullptr: none.
  // use_curv: DevModel::use_curv of the sweep; cw: curvature weight of the recursion (the arms: 0 or 1).
  // d_rec [B][N][rs], d_dz [B][N][nv], d_nu [B][N][nx], d_mu [B], d_ok [B]
  void (*fused_step_debug)(rmpc_handle *h, int B, const double *d_xinit, const double *d_x0, const double *d_params, int warm,
                           int use_curv, double cw, double *d_rec, double *d_dz, double *d_nu, double *d_mu, int *d_ok,
                           hipStream_t st);
  // test aid (rmpc_debug_step_curv): the recursion of the pass kernels at the weight cw on the records of the first
  // sweep.  k_riccati's path: d_ok [B] the recursion's return value, returns 0.  k_riccati_lane's (ric_lane as
  // launch_pass reads it): runs the kernel itself, d_ok [B] is 1 where the first pass cannot take that weight, returns 1.
  int (*pass_step_debug)(rmpc_handle *h, const Phase &ph, double cw, int *d_ok, hipStream_t st);
  void (*advance)(rmpc_handle *h, int B, const double *d_z_prev, const int *ef, double *d_xinit, double *d_x0,
                  int previous_plan, hipStream_t st);
  void (*retarget)(rmpc_handle *h, int B, const RetargetDev &R, hipStream_t st);
#if defined(RMPC_STAMPS) || defined(RMPC_RIC_STAMPS)
  int (*read_stamps)(int which, long long *out);   // reads and clears g_sst / g_rst (STAMPS_*) of the entry's unit
#endif
};
enum { STAMPS_SWEEP = 0, STAMPS_RIC = 1 };
void add_variant_ops(const VariantOps &v);   // rmpc_host.hip
