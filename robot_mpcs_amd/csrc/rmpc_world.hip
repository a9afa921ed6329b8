// rmpc_world.hip -- the world around the solver, on the device: the moving obstacles between two control steps, the
// free-space decomposition, the global planner (rmpc_grid.hpp), the lidar and the fleet's separating planes
// (rmpc_sense.hpp), the map built from the scans (rmpc_map.hpp), the assignment of robots to frontier targets
// (rmpc_assign.hpp), the minimum-cost assignment of robots to goals (rmpc_assign_opt.hpp, include/rmpc_assign_opt.h),
// tours of several tasks per robot and the follower that stops at them (rmpc_tours.hpp, include/rmpc_tours.h),
// localisation by scan matching (rmpc_locate.hpp), the fleet's timed routes (rmpc_timed.hpp), timed tours through
// every robot's stops (rmpc_timed_tours.hpp, include/rmpc_timed_tours.h), traffic-aware routes on a table of the fleet's
// flow (rmpc_traffic.hpp, include/rmpc_traffic.h), with
// their entries of the C ABI.  None of them
// takes a handle: each call runs on the device its first pointer lives on, on the stream it is given.  A translation
// unit of its own, which needs rmpc.h, the HIP runtime and the error channel only -- nothing of the solver.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <string>

#include "../../include/rmpc.h"
#include "../../include/rmpc_grid_large.h"
#include "../../include/rmpc_assign_opt.h"
#include "../../include/rmpc_tours.h"
#include "../../include/rmpc_timed_tours.h"
#include "../../include/rmpc_timed_replan.h"
#include "../../include/rmpc_timed_repair.h"
#include "../../include/rmpc_cbs.h"
#include "../../include/rmpc_ecbs.h"
#include "../../include/rmpc_any_angle.h"
#include "../../include/rmpc_corridor.h"
#include "../../include/rmpc_traffic.h"
#include "rmpc_err.hpp"

namespace rmpc {

// The environment of the moving obstacles between two control steps (what the examples' simulator does before the driver
// hands the planner ob[nx:], mpcPlanner.py:243-244): pos += vel dt + acc dt^2 / 2, vel += acc dt, one lane per
// (instance, obstacle); arena > 0: an obstacle that leaves [-arena, arena] in x or y comes back (velocity component
// mirrored), so that a loop that runs for hours keeps its obstacles.
static __global__ __launch_bounds__(256) void k_obst_advance(double *__restrict__ od, int n, double dt, double arena) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double *o = od + (size_t)i * 9;
  for (int c = 0; c < 3; c++) {
    double pos = o[c] + o[3 + c] * dt + 0.5 * o[6 + c] * dt * dt;
    double vel = o[3 + c] + o[6 + c] * dt;
    if (arena > 0.0 && c < 2) {
      if (pos > arena) { pos = 2.0 * arena - pos; vel = -vel; }
      else if (pos < -arena) { pos = -2.0 * arena - pos; vel = -vel; }
    }
    o[c] = pos; o[3 + c] = vel;
  }
}

// ===========================================================================
// Free-space decomposition: lidar point cloud -> at most K half-planes
// around a seed point, one lane per (instance, stage) seed.  Greedy rule of the reference
// (robotmpcs/utils/free_space_decomposition.py:79-97): the closest remaining point inside
// max_radius defines the plane through it with normal (seed - point); points on or behind the
// plane are discarded; unused slots get the dummy plane of asdict() (:110-114).  The sort of
// the reference is replaced by K arg-min sweeps over a keep-mask (P <= 64 points).
// ===========================================================================
__global__ __launch_bounds__(256) void k_fsd(const double *__restrict__ points, const double *__restrict__ seeds,
                                             double *__restrict__ out, int B, int N, int P, int K, double max_radius) {
#pragma clang fp contract(off)
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= B * N) return;
  const int b = gid / N;
  const double *pc = points + (size_t)b * P * 3;
  const double s0 = seeds[(size_t)gid * 3], s1 = seeds[(size_t)gid * 3 + 1], s2 = seeds[(size_t)gid * 3 + 2];
  double *o = out + (size_t)gid * K * 4;
  unsigned long long keep = 0ull;
  for (int i = 0; i < P; i++) {
    const double d0 = pc[3 * i] - s0, d1 = pc[3 * i + 1] - s1, d2 = pc[3 * i + 2] - s2;
    if (sqrt(d0 * d0 + d1 * d1 + d2 * d2) < max_radius) keep |= (1ull << i);
  }
  int nc = 0;
  while (keep && nc < K) {
    int best = -1;
    double bd = 0.0;
    for (int i = 0; i < P; i++)
      if (keep & (1ull << i)) {
        const double d0 = pc[3 * i] - s0, d1 = pc[3 * i + 1] - s1, d2 = pc[3 * i + 2] - s2;
        const double dd = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        if (best < 0 || dd < bd) { best = i; bd = dd; }
      }
    const double p0 = pc[3 * best], p1 = pc[3 * best + 1], p2 = pc[3 * best + 2];
    const double n0 = s0 - p0, n1 = s1 - p1, n2 = s2 - p2;
    const double c = -((n0 * p0 + n1 * p1) + n2 * p2);
    o[4 * nc] = n0; o[4 * nc + 1] = n1; o[4 * nc + 2] = n2; o[4 * nc + 3] = c;
    nc++;
    for (int i = 0; i < P; i++)
      if (keep & (1ull << i)) {
        const double v = ((n0 * pc[3 * i] + n1 * pc[3 * i + 1]) + n2 * pc[3 * i + 2]) + c;
        if (v <= 0.0) keep &= ~(1ull << i);
      }
  }
  for (; nc < K; nc++) {
    // HalfPlane(seed + (20, 20, 0), seed): normal = seed - point
    const double p0 = s0 + 20.0, p1 = s1 + 20.0, p2 = s2 + 0.0;
    const double n0 = s0 - p0, n1 = s1 - p1, n2 = s2 - p2;
    o[4 * nc] = n0; o[4 * nc + 1] = n1; o[4 * nc + 2] = n2; o[4 * nc + 3] = -((n0 * p0 + n1 * p1) + n2 * p2);
  }
}

}  // namespace rmpc

#include "rmpc_grid.hpp"
#include "rmpc_grid_large.hpp"
#include "rmpc_sense.hpp"
#include "rmpc_map.hpp"
#include "rmpc_assign.hpp"
#include "rmpc_assign_opt.hpp"
#include "rmpc_tours.hpp"
#include "rmpc_locate.hpp"
#include "rmpc_search.hpp"
#include "rmpc_timed.hpp"
#include "rmpc_timed_tours.hpp"
#include "rmpc_timed_replan.hpp"
#include "rmpc_timed_repair.hpp"
#include "rmpc_cbs.hpp"
#include "rmpc_ecbs.hpp"
#include "rmpc_track.hpp"
#include "rmpc_any_angle.hpp"
#include "rmpc_corridor.hpp"
#include "rmpc_traffic.hpp"

using namespace rmpc;

// no handle names the device: a call runs on the one this pointer lives on
static int use_device_of(const void *p) {
  hipPointerAttribute_t a;
  HIPCHK(hipPointerGetAttributes(&a, p));
  if (a.device < 0) return fail("not a device pointer");
  HIPCHK(hipSetDevice(a.device));
  return 0;
}
// what every entry ends with, behind its launch
static int launch_status() {
  HIPCHK(hipGetLastError());
  return 0;
}

/* the global planner (rmpc_grid.hpp): no handle; each call runs on the device its first pointer lives on */
static bool grid_fits(long long a, long long b) { return a >= 0 && b >= 0 && (b == 0 || a <= INT_MAX / b); }
static int grid_check(int H, int W, int movement) {
  if (H < 1 || W < 1 || !grid_fits(H, W)) return fail("grid: need H, W >= 1");
  if (movement != 4 && movement != 8) return fail("grid: movement must be 4 or 8");
  return 0;
}
// The checks several entries make, each under the entry's prefix `who`.  A map of more than RMPC_GRID_MAX_CELLS cells
// (or of none) is refused in one of two wordings: `sized` names the map's size (the fields, behind grid_check).
static int grid_cells_check(const std::string &who, int H, int W, bool sized) {
  if (H >= 1 && W >= 1 && grid_fits(H, W) && H * W <= RMPC_GRID_MAX_CELLS) return 0;
  const std::string max = "RMPC_GRID_MAX_CELLS = " + std::to_string(RMPC_GRID_MAX_CELLS);
  if (!sized) return fail(who + ": need H, W >= 1 and H*W <= " + max);
  return fail(who + ": " + std::to_string(H) + "x" + std::to_string(W) + " map exceeds " + max +
              " cells (one field must fit in the LDS of a workgroup)");
}
static int grid_fields_check(const std::string &who, int G, int H, int W) {
  return G < 1 || !grid_fits(G, (long long)H * W) ? fail(who + ": need 1 <= G and G*H*W <= INT_MAX") : 0;
}
static int grid_paths_check(const std::string &who, int B, int max_len) {
  return B < 1 || max_len < 1 || !grid_fits(B, max_len) ? fail(who + ": need B, max_len >= 1 and B*max_len <= INT_MAX") : 0;
}
static int grid_cost_check(const std::string &who, double cost_factor) {
  return !(cost_factor >= 0.0) || std::isinf(cost_factor) ? fail(who + ": cost_factor must be finite and >= 0") : 0;
}

// rmpc_grid_fields_device and rmpc_grid_fields_seeded_device (both speak as "grid fields"): `d_src` the goal cells or
// the seed grids of `kernel`
template <class Kernel, class T>
static int grid_fields(Kernel kernel, int H, int W, const double *d_grid, int G, const T *d_src, int movement,
                       double occ_threshold, double cost_factor, double *d_fields, int32_t *d_status, int32_t *d_sweeps,
                       void *stream) {
  const char *who = "grid fields";
  if (!d_grid || !d_src || !d_fields || !d_status) return fail("null argument");
  if (grid_check(H, W, movement) || grid_cells_check(who, H, W, true) || grid_fields_check(who, G, H, W) ||
      grid_cost_check(who, cost_factor) || use_device_of(d_grid))
    return -1;
  hipLaunchKernelGGL(kernel, dim3(G), dim3(kGridThreads), 0, (hipStream_t)stream, d_grid, H, W, d_src, movement,
                     occ_threshold, cost_factor, d_fields, (int *)d_status, (int *)d_sweeps);
  return launch_status();
}

// rmpc_grid_fields_large_device and rmpc_grid_fields_seeded_large_device (include/rmpc_grid_large.h; both speak as
// "grid fields large"): every refusal comes before the first HIP call
template <bool kSeeded>
static int grid_fields_large(int H, int W, const double *d_grid, int G, const int *d_goal_cells, const double *d_seeds,
                             int movement, double occ_threshold, double cost_factor, double *d_fields,
                             int32_t *d_status, int32_t *d_visits, void *stream) {
  const std::string who = "grid fields large";
  if (!d_grid || !(kSeeded ? (const void *)d_seeds : (const void *)d_goal_cells) || !d_fields || !d_status)
    return fail("null argument");
  if (H < 1 || W < 1) return fail(who + ": need H, W >= 1");
  if (movement != 4 && movement != 8) return fail(who + ": movement must be 4 or 8");
  if (H > RMPC_GRID_LARGE_MAX_SIDE || W > RMPC_GRID_LARGE_MAX_SIDE)
    return fail(who + ": " + std::to_string(H) + "x" + std::to_string(W) + " map has a side above RMPC_GRID_LARGE_MAX_SIDE = " +
                std::to_string(RMPC_GRID_LARGE_MAX_SIDE));
  if ((long long)H * W > RMPC_GRID_LARGE_MAX_CELLS)
    return fail(who + ": " + std::to_string(H) + "x" + std::to_string(W) + " map exceeds RMPC_GRID_LARGE_MAX_CELLS = " +
                std::to_string(RMPC_GRID_LARGE_MAX_CELLS) + " cells");
  if (grid_fields_check(who, G, H, W) || grid_cost_check(who, cost_factor) || use_device_of(d_grid)) return -1;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_grid_fields_large<kSeeded>), dim3(G), dim3(kLargeThreads), 0, (hipStream_t)stream,
                     d_grid, H, W, d_goal_cells, d_seeds, movement, occ_threshold, cost_factor, d_fields, (int *)d_status,
                     (int *)d_visits);
  return launch_status();
}

// rmpc_grid_paths_device and rmpc_grid_descend_device: `d_ends` the goal cells or the seed grids of `kernel`
template <class Kernel, class T>
static int grid_descent(const char *who, Kernel kernel, int H, int W, const double *d_grid, int G, const double *d_fields,
                        const T *d_ends, int B, const int32_t *d_start_cell, const int32_t *d_index, int movement,
                        double occ_threshold, double cost_factor, int max_len, int32_t *d_path, int32_t *d_len,
                        void *stream) {
  if (!d_grid || !d_fields || !d_ends || !d_start_cell || !d_index || !d_path || !d_len) return fail("null argument");
  if (grid_check(H, W, movement) || grid_fields_check(who, G, H, W) || grid_paths_check(who, B, max_len) ||
      grid_cost_check(who, cost_factor) || use_device_of(d_grid))
    return -1;
  hipLaunchKernelGGL(kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_grid, H, W, d_fields, d_ends, G,
                     (const int *)d_start_cell, (const int *)d_index, B, movement, occ_threshold, cost_factor, max_len,
                     (int *)d_path, (int *)d_len);
  return launch_status();
}

// rmpc_timed_plan_device, rmpc_timed_tours_plan_device and rmpc_timed_tours_replan_device: one workgroup per order of
// a planner kernel, `lds` with the history in LDS where it fits, `mem` with it in the workspace beyond.  It stands here,
// with the other launch templates and not in the timed block below, because a template cannot lie inside extern "C".
template <class Kernel, class... Args>
static void timed_launch(Kernel lds, Kernel mem, int G, int T, const TimedGeom &q, void *stream, Args... args) {
  const size_t hist = (size_t)(T + 1) * q.L * sizeof(timed_word);
  const int nt = q.L <= 64 ? 64 : (q.L <= 128 ? 128 : kTimedThreads);      // a power of two: the end cell's reduction
  if (hist <= (size_t)kTimedHistLds) hipLaunchKernelGGL(lds, dim3(G), dim3(nt), hist, (hipStream_t)stream, args...);
  else hipLaunchKernelGGL(mem, dim3(G), dim3(nt), 0, (hipStream_t)stream, args...);
}

// rmpc_ecbs_device: the history in LDS as timed_launch decides it, the three int32 rows of H W cells behind it when
// they are small; the workgroup is timed_launch's
template <class Kernel, class... Args>
static void ecbs_launch(Kernel both, Kernel hist, Kernel rows, Kernel none, int G, int H, int W, int T, const TimedGeom &q,
                        void *stream, Args... args) {
  const size_t hb = (size_t)(T + 1) * q.L * sizeof(timed_word), rb = 3 * sizeof(int) * (size_t)H * W;
  const bool hl = hb <= (size_t)kTimedHistLds, rl = rb <= (size_t)kEcbsRowsLds;
  const int nt = q.L <= 64 ? 64 : (q.L <= 128 ? 128 : kTimedThreads);
  const Kernel kernel = hl ? (rl ? both : hist) : (rl ? rows : none);
  const size_t lds = (hl ? hb : 0) + (rl ? rb : 0);            // up to 100 KB beside 14 KB of static LDS
  if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, dim3(G), dim3(nt), lds, (hipStream_t)stream, args...);
}

extern "C" {

int rmpc_advance_obstacles_device(int B, int nobst, double dt, double arena, double *d_obst_dyn, void *stream) {
  if (B < 1 || nobst < 1 || !d_obst_dyn) return fail("bad argument");
  const int n = B * nobst;
  hipLaunchKernelGGL(k_obst_advance, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_obst_dyn, n, dt, arena);
  return launch_status();
}

int rmpc_free_space_device(int B, int N, int P, int K, double max_radius, const double *d_points,
                           const double *d_seeds, double *d_planes, void *stream) {
  if (!d_points || !d_seeds || !d_planes) return fail("null argument");
  if (B < 1 || N < 1 || K < 1 || P < 1 || P > 64) return fail("free space decomposition: need 1 <= P <= 64 points, K >= 1");
  if (use_device_of(d_points)) return -1;
  hipLaunchKernelGGL(k_fsd, dim3((B * N + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_points, d_seeds, d_planes,
                     B, N, P, K, max_radius);
  return launch_status();
}

/* the global planner's entries (rmpc_grid.hpp) */
int rmpc_grid_inflate_device(int H, int W, double cell, double size_robot, double threshold, const double *d_grid,
                             double *d_out, void *stream) {
  if (!d_grid || !d_out) return fail("null argument");
  if (grid_check(H, W, 8) || use_device_of(d_grid)) return -1;
  if (!(cell > 0.0) || !(size_robot >= 0.0)) return fail("grid inflate: need cell > 0, size_robot >= 0");
  const double kd = ceil(size_robot / cell);
  if (kd > (double)(H + W)) return fail("grid inflate: window larger than the map");
  hipLaunchKernelGGL(k_grid_inflate, dim3((H * W + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_grid, d_out, H, W,
                     (int)kd, threshold);
  return launch_status();
}

int rmpc_grid_fields_device(int H, int W, const double *d_grid, int G, const int32_t *d_goal_cells, int movement,
                            double occ_threshold, double cost_factor, double *d_fields, int32_t *d_status,
                            int32_t *d_sweeps, void *stream) {
  return grid_fields(k_grid_fields, H, W, d_grid, G, (const int *)d_goal_cells, movement, occ_threshold, cost_factor,
                     d_fields, d_status, d_sweeps, stream);
}

int rmpc_grid_fields_seeded_device(int H, int W, const double *d_grid, int G, const double *d_seeds, int movement,
                                   double occ_threshold, double cost_factor, double *d_fields, int32_t *d_status,
                                   int32_t *d_sweeps, void *stream) {
  return grid_fields(k_grid_fields_seeded, H, W, d_grid, G, d_seeds, movement, occ_threshold, cost_factor, d_fields,
                     d_status, d_sweeps, stream);
}

int rmpc_grid_fields_large_device(int H, int W, const double *d_grid, int G, const int32_t *d_goal_cells, int movement,
                                  double occ_threshold, double cost_factor, double *d_fields, int32_t *d_status,
                                  int32_t *d_visits, void *stream) {
  return grid_fields_large<false>(H, W, d_grid, G, (const int *)d_goal_cells, nullptr, movement, occ_threshold, cost_factor,
                                  d_fields, d_status, d_visits, stream);
}

int rmpc_grid_fields_seeded_large_device(int H, int W, const double *d_grid, int G, const double *d_seeds, int movement,
                                         double occ_threshold, double cost_factor, double *d_fields, int32_t *d_status,
                                         int32_t *d_visits, void *stream) {
  return grid_fields_large<true>(H, W, d_grid, G, nullptr, d_seeds, movement, occ_threshold, cost_factor, d_fields,
                                 d_status, d_visits, stream);
}

int rmpc_grid_paths_device(int H, int W, const double *d_grid, int G, const double *d_fields, const int32_t *d_goal_cells,
                           int B, const int32_t *d_start_cell, const int32_t *d_goal_index, int movement,
                           double occ_threshold, double cost_factor, int max_len, int32_t *d_path, int32_t *d_len,
                           void *stream) {
  return grid_descent("grid paths", k_grid_paths, H, W, d_grid, G, d_fields, (const int *)d_goal_cells, B, d_start_cell,
                      d_goal_index, movement, occ_threshold, cost_factor, max_len, d_path, d_len, stream);
}

int rmpc_grid_descend_device(int H, int W, const double *d_grid, int G, const double *d_fields, const double *d_seeds,
                             int B, const int32_t *d_start_cell, const int32_t *d_field_index, int movement,
                             double occ_threshold, double cost_factor, int max_len, int32_t *d_path, int32_t *d_len,
                             void *stream) {
  return grid_descent("grid descend", k_grid_descend, H, W, d_grid, G, d_fields, d_seeds, B, d_start_cell, d_field_index,
                      movement, occ_threshold, cost_factor, max_len, d_path, d_len, stream);
}

int rmpc_grid_cells_device(int B, const double *d_pos, int stride, int H, int W, double x0, double y0, double cell,
                           int32_t *d_cells, void *stream) {
  if (!d_pos || !d_cells) return fail("null argument");
  if (B < 1 || stride < 2 || !grid_fits(B, stride)) return fail("grid cells: need B >= 1, stride >= 2, B*stride <= INT_MAX");
  if (grid_check(H, W, 8) || use_device_of(d_pos)) return -1;
  if (!(cell > 0.0)) return fail("grid cells: need cell > 0");
  hipLaunchKernelGGL(k_grid_cells, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_pos, stride, B, H, W, x0,
                     y0, cell, (int *)d_cells);
  return launch_status();
}

int rmpc_follow_path_device(int B, const int32_t *d_path, const int32_t *d_len, int max_len, int32_t *d_idx,
                            const double *d_pos, int stride, int W, double x0, double y0, double cell, double threshold,
                            double *d_goal, void *stream) {
  if (!d_path || !d_len || !d_idx || !d_pos || !d_goal) return fail("null argument");
  if (grid_paths_check("follow path", B, max_len)) return -1;
  if (stride < 2 || !grid_fits(B, stride) || W < 1) return fail("follow path: need stride >= 2, W >= 1");
  if (use_device_of(d_path)) return -1;
  hipLaunchKernelGGL(k_follow_path, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const int *)d_path,
                     (const int *)d_len, max_len, (int *)d_idx, d_pos, stride, B, W, x0, y0, cell, threshold, d_goal);
  return launch_status();
}

/* the lidar (rmpc_sense.hpp): no handle; each call runs on the device its first pointer lives on */
static int lidar_scan_check(int B, const rmpc_lidar *l) {
  if (!l) return fail("null argument");
  if (l->struct_size != (int)sizeof(rmpc_lidar)) return fail("rmpc_lidar.struct_size mismatch");
  if (B < 1 || l->rays < 1) return fail("lidar: need B >= 1 and rays >= 1");
  if (l->pose_stride < 3) return fail("lidar: pose_stride must be >= 3 (x, y, heading)");
  if (l->nbox < 0 || l->ncircle < 0) return fail("lidar: negative shape count");
  if (!grid_fits(B, l->rays) || !grid_fits(B, l->pose_stride) || !grid_fits(l->nbox, 4) || !grid_fits(l->ncircle, 3))
    return fail("lidar: B*rays, B*pose_stride, nbox*4 and ncircle*3 must not exceed INT_MAX");
  if (!(l->range > 0.0) || std::isinf(l->range)) return fail("lidar: range must be positive and finite");
  if (!l->pose || !l->points || (l->nbox > 0 && !l->boxes) || (l->ncircle > 0 && !l->circles)) return fail("null argument");
  return 0;
}

int rmpc_lidar_scan_device(int B, const rmpc_lidar *l, void *stream) {
  if (lidar_scan_check(B, l) || use_device_of(l->pose)) return -1;
  const int n = B * l->rays;
  const double step = (l->angle_max - l->angle_min) / (double)l->rays;
  hipLaunchKernelGGL(k_lidar, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, l->pose, l->pose_stride, B,
                     l->rays, l->angle_min, step, l->range, l->offset_x, l->offset_y, l->height, l->boxes, l->nbox,
                     l->circles, l->ncircle, l->points, l->ranges);
  return launch_status();
}

/* the fleet in the scan (k_lidar_fleet): one workgroup per robot, as wide as its rays need (64 .. 256) */
int rmpc_lidar_scan_fleet_device(int B, const rmpc_lidar *l, const rmpc_lidar_bodies *f, void *stream) {
  if (!f) return fail("null argument");
  if (f->struct_size != (int)sizeof(rmpc_lidar_bodies)) return fail("rmpc_lidar_bodies.struct_size mismatch");
  if (lidar_scan_check(B, l)) return -1;
  if (f->P < 0) return fail("lidar fleet: negative body count");
  if (f->centre_stride < 2) return fail("lidar fleet: centre_stride must be >= 2 (cx, cy)");
  if (!grid_fits(f->P, f->centre_stride)) return fail("lidar fleet: P*centre_stride must not exceed INT_MAX");
  if (f->P > 0 && (!f->centres || !f->radius)) return fail("null argument");
  if (use_device_of(l->pose)) return -1;
  const double step = (l->angle_max - l->angle_min) / (double)l->rays;
  const int threads = l->rays <= 64 ? 64 : l->rays <= 128 ? 128 : 256;
  hipLaunchKernelGGL(k_lidar_fleet, dim3(B), dim3(threads), 0, (hipStream_t)stream, l->pose, l->pose_stride, l->rays,
                     l->angle_min, step, l->range, l->offset_x, l->offset_y, l->height, l->boxes, l->nbox, l->circles,
                     l->ncircle, f->centres, f->centre_stride, f->radius, f->P, f->self0, l->points, l->ranges,
                     f->static_ranges, (int *)f->owner);
  return launch_status();
}

static int plan_points(int B, int N, const double *d_z_prev, int nvar, const int32_t *d_exitflag, const double *d_pose,
                       int pose_stride, int shift, int heading, double offset_x, double offset_y, double height,
                       double *d_points, void *stream) {
  if (!d_pose || !d_points) return fail("null argument");
  if (B < 1 || N < 1) return fail("plan points: need B, N >= 1");
  if (heading != 0 && heading != 1) return fail("plan points: heading must be 0 or 1");
  if (pose_stride < 3) return fail("plan points: pose_stride must be >= 3 (x, y, heading)");
  if (nvar < 3) return fail("plan points: nvar must be >= 3 (x, y, heading first)");
  if (!grid_fits(B, N) || !grid_fits(B, pose_stride) || !grid_fits((long long)B * N, nvar))
    return fail("plan points: B*N, B*pose_stride and B*N*nvar must not exceed INT_MAX");
  if (use_device_of(d_z_prev ? (const void *)d_z_prev : (const void *)d_pose)) return -1;
  hipLaunchKernelGGL(k_plan_points, dim3((B * N + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_z_prev, nvar,
                     (const int *)d_exitflag, d_pose, pose_stride, B, N, shift, heading, offset_x, offset_y, height,
                     d_points);
  return launch_status();
}

int rmpc_plan_points_device(int B, int N, const double *d_z_prev, int nvar, const int32_t *d_exitflag,
                            const double *d_pose, int pose_stride, double offset_x, double offset_y, double height,
                            double *d_points, void *stream) {
  return plan_points(B, N, d_z_prev, nvar, d_exitflag, d_pose, pose_stride, 0, 1, offset_x, offset_y, height, d_points,
                     stream);
}

/* fleet separation (rmpc_sense.hpp): no handle; each call runs on the device its first pointer lives on */
int rmpc_fleet_points_device(int B, int N, const double *d_z_prev, int nvar, const int32_t *d_exitflag,
                             const double *d_pose, int pose_stride, int heading, double offset_x, double offset_y,
                             double height, double *d_points, void *stream) {
  return plan_points(B, N, d_z_prev, nvar, d_exitflag, d_pose, pose_stride, 1, heading, offset_x, offset_y, height,
                     d_points, stream);
}

int rmpc_fleet_planes_device(int B, int N, const double *d_points, const double *d_radius, int K, double range,
                             int nobst, int slot0, double *d_planes, void *stream) {
  if (!d_points || !d_radius || !d_planes) return fail("null argument");
  if (B < 1 || N < 1) return fail("fleet planes: need B, N >= 1");
  if (K < 1 || K > rmpc::kFleetKMax) return fail("fleet planes: need 1 <= K <= 8");
  if (slot0 < 0 || nobst < 1 || slot0 > nobst - K) return fail("fleet planes: need 0 <= slot0 and slot0 + K <= nobst");
  if (!(range >= 0.0)) return fail("fleet planes: range must be >= 0 (+inf admits every robot)");
  if (!grid_fits(B, N) || !grid_fits((long long)B * N, nobst) || !grid_fits((long long)B * N * nobst, 4))
    return fail("fleet planes: B*N*nobst*4 must not exceed INT_MAX");
  if (use_device_of(d_points)) return -1;
  const int nbt = (B + 255) / 256;
  hipLaunchKernelGGL(k_fleet_planes, dim3(nbt * N), dim3(256), 0, (hipStream_t)stream, d_points, d_radius, B, N, K,
                     range * range, nobst, slot0, d_planes);
  return launch_status();
}

/* the map from the scans (rmpc_map.hpp): no handle; each call runs on the device its first pointer lives on */
int rmpc_grid_mark_device(int B, const rmpc_grid_mark *m, void *stream) {
  if (!m) return fail("null argument");
  if (m->struct_size != (int)sizeof(rmpc_grid_mark)) return fail("rmpc_grid_mark.struct_size mismatch");
  if (B < 1 || m->rays < 1) return fail("grid mark: need B >= 1 and rays >= 1");
  if (!grid_fits(B, m->rays) || !grid_fits((long long)B * m->rays, 3)) return fail("grid mark: B*rays*3 must not exceed INT_MAX");
  if (grid_cells_check("grid mark", m->H, m->W, false)) return -1;
  if (!(m->cell > 0.0) || std::isinf(m->cell) || !(m->range > 0.0) || std::isinf(m->range))
    return fail("grid mark: cell and range must be positive and finite");
  if (!(m->hit_depth >= 0.0) || std::isinf(m->hit_depth)) return fail("grid mark: hit_depth must be finite and >= 0");
  if (!std::isfinite(m->x0) || !std::isfinite(m->y0)) return fail("grid mark: x0, y0 must be finite");
  if (!m->origins || !m->points || !m->ranges || !m->hits || !m->misses) return fail("null argument");
  const double reach = ceil((m->range + m->hit_depth) / m->cell);
  if (!(2.0 * reach + 4.0 <= 1073741824.0)) return fail("grid mark: (range + hit_depth) / cell must not exceed 2^29 cells");
  if (use_device_of(m->origins)) return -1;
  MapGeom g;
  g.H = m->H; g.W = m->W; g.x0 = m->x0; g.y0 = m->y0; g.cell = m->cell; g.range = m->range; g.hit_depth = m->hit_depth;
  g.nmax = 2.0 * reach + 4.0;
  const int R = m->rays;
  hipLaunchKernelGGL(k_grid_mark, dim3((B * R + 255) / 256), dim3(256), 0, (hipStream_t)stream, m->origins, m->points,
                     m->ranges, B, R, g, (int *)m->hits, (int *)m->misses, (int *)m->skipped);
  return launch_status();
}

int rmpc_grid_occupancy_device(int H, int W, int32_t *d_hits, int32_t *d_misses, int w_hit, int w_miss, int forget,
                               double free_value, double occ_value, double unknown_value, double *d_grid, void *stream) {
  if (!d_hits || !d_misses || !d_grid) return fail("null argument");
  if (grid_cells_check("grid occupancy", H, W, false)) return -1;
  if (w_hit < 1 || w_miss < 1) return fail("grid occupancy: need w_hit, w_miss >= 1");
  if (forget < 0 || forget > 31) return fail("grid occupancy: forget must lie in [0, 31]");
  if (!std::isfinite(free_value) || !std::isfinite(occ_value) || !std::isfinite(unknown_value))
    return fail("grid occupancy: the three values must be finite");
  if (use_device_of(d_hits)) return -1;
  hipLaunchKernelGGL(k_grid_occupancy, dim3((H * W + 255) / 256), dim3(256), 0, (hipStream_t)stream, H * W, (int *)d_hits,
                     (int *)d_misses, w_hit, w_miss, forget, free_value, occ_value, unknown_value, d_grid);
  return launch_status();
}

/* the frontier of the map (rmpc_map.hpp) */
int rmpc_grid_frontier_device(int H, int W, const int32_t *d_hits, const int32_t *d_misses, const double *d_enlarged,
                              double occ_threshold, int nmoves, double unknown_value, double *d_plan, double *d_seed,
                              int32_t *d_count, void *stream) {
  if (!d_hits || !d_misses || !d_enlarged || !d_plan || !d_seed || !d_count) return fail("null argument");
  if (grid_cells_check("grid frontier", H, W, false)) return -1;
  if (nmoves != 4 && nmoves != 8) return fail("grid frontier: nmoves must be 4 or 8");
  if (!std::isfinite(occ_threshold) || !std::isfinite(unknown_value))
    return fail("grid frontier: occ_threshold and unknown_value must be finite");
  if (use_device_of(d_hits)) return -1;
  hipLaunchKernelGGL(k_grid_frontier, dim3((H * W + 255) / 256), dim3(256), 0, (hipStream_t)stream, H, W,
                     (const int *)d_hits, (const int *)d_misses, d_enlarged, occ_threshold, nmoves, unknown_value, d_plan,
                     d_seed, (int *)d_count);
  return launch_status();
}

/* coordinated exploration (rmpc_assign.hpp) */
int rmpc_grid_targets_device(int H, int W, const double *d_seed, int tile, int32_t *d_target_cells, double *d_tseeds,
                             void *stream) {
  if (!d_seed || !d_target_cells) return fail("null argument");
  if (grid_cells_check("grid targets", H, W, false)) return -1;
  if (tile < 1) return fail("grid targets: need tile >= 1");
  const long long ntr = ((long long)H + tile - 1) / tile, ntc = ((long long)W + tile - 1) / tile;
  if (ntr * ntc > RMPC_ASSIGN_MAX_TARGETS)
    return fail("grid targets: " + std::to_string(ntr * ntc) + " tiles exceed RMPC_ASSIGN_MAX_TARGETS = " +
                std::to_string(RMPC_ASSIGN_MAX_TARGETS));
  if (use_device_of(d_seed)) return -1;
  hipLaunchKernelGGL(k_grid_targets, dim3((int)(ntr * ntc)), dim3(256), 0, (hipStream_t)stream, H, W, d_seed, tile,
                     (int)ntc, (int *)d_target_cells, d_tseeds);
  return launch_status();
}

static int assign_sizes_check(const std::string &who, int B, int T) {
  if (B >= 1 && B <= RMPC_ASSIGN_MAX_ROBOTS && T >= 1 && T <= RMPC_ASSIGN_MAX_TARGETS) return 0;
  return fail(who + ": need 1 <= B <= RMPC_ASSIGN_MAX_ROBOTS = " + std::to_string(RMPC_ASSIGN_MAX_ROBOTS) +
              " and 1 <= T <= RMPC_ASSIGN_MAX_TARGETS = " + std::to_string(RMPC_ASSIGN_MAX_TARGETS));
}

int rmpc_grid_route_costs_device(int H, int W, const double *d_grid, int T, const double *d_fields, int B,
                                 const int32_t *d_start_cell, int movement, double occ_threshold, double cost_factor,
                                 double *d_cost, void *stream) {
  const char *who = "grid route costs";
  if (!d_grid || !d_fields || !d_start_cell || !d_cost) return fail("null argument");
  if (grid_check(H, W, movement) || assign_sizes_check(who, B, T) || grid_fields_check(who, T, H, W) ||
      grid_cost_check(who, cost_factor) || use_device_of(d_grid))
    return -1;
  hipLaunchKernelGGL(k_grid_route_costs, dim3((B * T + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_grid, H, W, T,
                     d_fields, B, (const int *)d_start_cell, movement, occ_threshold, cost_factor, d_cost);
  return launch_status();
}

int rmpc_assign_greedy_device(int B, int T, const double *d_cost, int32_t *d_assign, int32_t *d_pass, void *stream) {
  if (!d_cost || !d_assign) return fail("null argument");
  if (assign_sizes_check("assign greedy", B, T) || use_device_of(d_cost)) return -1;
  hipLaunchKernelGGL(k_assign_greedy, dim3(1), dim3(kAssignThreads), 0, (hipStream_t)stream, B, T, d_cost,
                     (int *)d_assign, (int *)d_pass);
  return launch_status();
}

/* minimum-cost assignment (rmpc_assign_opt.hpp, include/rmpc_assign_opt.h) */
static int assign_opt_sizes_check(const std::string &who, int G, int B, int T) {
  if (assign_sizes_check(who, B, T)) return -1;
  return G < 1 || !grid_fits(G, (long long)B * T) ? fail(who + ": need 1 <= G and G*B*T <= INT_MAX") : 0;
}

int64_t rmpc_assign_optimal_work_bytes(int G, int B, int T) {
  if (assign_opt_sizes_check("assign optimal work bytes", G, B, T)) return -1;
  return (int64_t)assign_opt_matrix_offset(G) + (int64_t)G * B * T * (int64_t)sizeof(int32_t);
}

int rmpc_assign_optimal_device(int G, int B, int T, const double *d_cost, double scale, int32_t *d_assign,
                               int64_t *d_total, int32_t *d_count, int32_t *d_steps, void *d_work,
                               int64_t work_bytes, void *stream) {
  const std::string who = "assign optimal";
  if (!d_cost || !d_assign || !d_work) return fail("null argument");
  if (assign_opt_sizes_check(who, G, B, T)) return -1;
  if (!(scale > 0.0) || std::isinf(scale)) return fail(who + ": scale must be finite and > 0");
  const int64_t need = rmpc_assign_optimal_work_bytes(G, B, T);
  if (work_bytes < need)
    return fail(who + ": the workspace holds " + std::to_string(work_bytes) + " bytes, " + std::to_string(need) +
                " are needed (rmpc_assign_optimal_work_bytes)");
  if (use_device_of(d_cost)) return -1;
  int *const qmax = (int *)d_work, *const Q = (int *)((char *)d_work + assign_opt_matrix_offset(G));
  const long long total = (long long)G * B * T;
  const int n = B <= T ? T : B;
  HIPCHK(hipMemsetAsync(qmax, 0, (size_t)G * sizeof(int), (hipStream_t)stream));
  hipLaunchKernelGGL(k_assign_quantise, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, T,
                     total, d_cost, scale, qmax, Q);
  // a thread per column up to 1024 columns, whole wavefronts; beyond that 2 or 4 columns per thread
  const int threads = n > 1024 ? 1024 : (n + 63) / 64 * 64;
  auto solve = n <= 64 ? k_assign_optimal<64, 1> : n <= 1024 ? k_assign_optimal<1024, 1>
               : n <= 2048 ? k_assign_optimal<1024, 2> : k_assign_optimal<1024, 4>;
  hipLaunchKernelGGL(solve, dim3(G), dim3(threads), 0, (hipStream_t)stream, B, T, (const int *)qmax, (const int *)Q,
                     (int *)d_assign, (long long *)d_total, (int *)d_count, (int *)d_steps);
  return launch_status();
}

/* tours of several tasks per robot (rmpc_tours.hpp, include/rmpc_tours.h) */
static int tours_sizes_check(const std::string &who, int G, int B, int T) {
  if (B < 1 || B > RMPC_TOURS_MAX_ROBOTS || T < 1 || T > RMPC_TOURS_MAX_TASKS)
    return fail(who + ": need 1 <= B <= RMPC_TOURS_MAX_ROBOTS = " + std::to_string(RMPC_TOURS_MAX_ROBOTS) +
                " and 1 <= T <= RMPC_TOURS_MAX_TASKS = " + std::to_string(RMPC_TOURS_MAX_TASKS));
  return G < 1 || !grid_fits(G, (long long)T * T) || !grid_fits(G, (long long)B * T)
             ? fail(who + ": need 1 <= G, G*T*T <= INT_MAX and G*B*T <= INT_MAX") : 0;
}

int64_t rmpc_tours_work_bytes(int G, int B, int T) {
  if (tours_sizes_check("tours work bytes", G, B, T)) return -1;
  return (int64_t)tours_work_ints(G, B, T) * (int64_t)sizeof(int32_t);
}

int rmpc_tours_device(int G, int B, int T, int K, const double *d_start_cost, const double *d_task_cost, int mode,
                      double scale, int max_rounds, int32_t *d_tours, int32_t *d_len, int64_t *d_cost, int32_t *d_owner,
                      int32_t *d_count, int64_t *d_total, int64_t *d_span, int32_t *d_build_steps, int32_t *d_rounds,
                      void *d_work, int64_t work_bytes, void *stream) {
  const std::string who = "tours";
  if (!d_start_cost || !d_task_cost || !d_tours || !d_len || !d_cost || !d_work) return fail("null argument");
  if (tours_sizes_check(who, G, B, T)) return -1;
  if (K < 1 || K > T) return fail(who + ": need 1 <= K <= T");
  if (mode != 0 && mode != 1) return fail(who + ": mode must be 0 (least sum) or 1 (least makespan)");
  if (!(scale > 0.0) || std::isinf(scale)) return fail(who + ": scale must be finite and > 0");
  if (max_rounds < 0) return fail(who + ": max_rounds must be >= 0");
  const int64_t need = rmpc_tours_work_bytes(G, B, T);
  if (work_bytes < need)
    return fail(who + ": the workspace holds " + std::to_string(work_bytes) + " bytes, " + std::to_string(need) +
                " are needed (rmpc_tours_work_bytes)");
  if (use_device_of(d_start_cost)) return -1;
  const long long nstart = (long long)G * B * T, ntask = (long long)G * T * T, total = nstart + ntask;
  int *const qs = (int *)d_work, *const qt = qs + nstart, *const qtT = qt + ntask, *const ins = qtT + ntask,
            *const pos = ins + nstart;
  hipLaunchKernelGGL(k_tours_quantise, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, T, nstart,
                     total, d_start_cost, d_task_cost, scale, qs, qt, qtT, ins, pos);
  // a thread per task, whole wavefronts; up to 64 tasks the workgroup is one wave
  auto solve = T <= 64 ? k_tours<64> : k_tours<1024>;
  hipLaunchKernelGGL(solve, dim3(G), dim3((T + 63) / 64 * 64), 0, (hipStream_t)stream, B, T, K, mode, max_rounds,
                     (const int *)qs, (const int *)qt, (const int *)qtT, ins, pos, (int *)d_tours, (int *)d_len, (long long *)d_cost,
                     (int *)d_owner, (int *)d_count, (long long *)d_total, (long long *)d_span, (int *)d_build_steps,
                     (int *)d_rounds);
  return launch_status();
}

int rmpc_follow_tour_device(int B, const int32_t *d_path, const int32_t *d_len, int max_len, int32_t *d_idx,
                            const double *d_pos, int stride, int W, double x0, double y0, double cell, double threshold,
                            double *d_goal, int K, const int32_t *d_stop_at, int32_t *d_leg, int32_t *d_served, int now,
                            double stop_tol, void *stream) {
  if (!d_path || !d_len || !d_idx || !d_pos || !d_goal || !d_stop_at || !d_leg || !d_served) return fail("null argument");
  if (grid_paths_check("follow tour", B, max_len)) return -1;
  if (K < 1 || !grid_fits(B, K)) return fail("follow tour: need K >= 1 and B*K <= INT_MAX");
  if (stride < 2 || !grid_fits(B, stride) || W < 1) return fail("follow tour: need stride >= 2, W >= 1");
  if (!(stop_tol >= 0.0)) return fail("follow tour: stop_tol must be >= 0");
  if (use_device_of(d_path)) return -1;
  hipLaunchKernelGGL(k_follow_tour, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const int *)d_path,
                     (const int *)d_len, max_len, (int *)d_idx, d_pos, stride, B, W, x0, y0, cell, threshold, d_goal, K,
                     (const int *)d_stop_at, (int *)d_leg, (int *)d_served, now, stop_tol);
  return launch_status();
}

/* localisation (rmpc_locate.hpp) */
static int edge_table_check(const std::string &who, int H, int W, int sub, int cap) {
  if (grid_cells_check(who, H, W, false)) return -1;
  if (sub < 1 || sub > 8) return fail(who + ": sub must lie in [1, 8]");
  if (cap < 1 || cap > 65535) return fail(who + ": cap must lie in [1, 65535]");
  return 0;
}

int rmpc_grid_edge_distance_device(int H, int W, const double *d_grid, double occ_threshold, int sub, int cap,
                                   int32_t *d_d2, void *stream) {
  if (!d_grid || !d_d2) return fail("null argument");
  if (edge_table_check("grid edge distance", H, W, sub, cap)) return -1;
  if (!std::isfinite(occ_threshold)) return fail("grid edge distance: occ_threshold must be finite");
  if (use_device_of(d_grid)) return -1;
  const int win = (int)ceil(sqrt((double)cap));                       // <= kEdgeMaxWin at cap <= 65535
  const int ntile = (W * sub + kEdgeTile - 1) / kEdgeTile;
  hipLaunchKernelGGL(k_edge_distance, dim3(H * sub * ntile), dim3(256), 0, (hipStream_t)stream, d_grid, H, W, occ_threshold,
                     sub, cap, win, ntile, (int *)d_d2);
  return launch_status();
}

int rmpc_lidar_project_device(int B, const rmpc_lidar *l, void *stream) {
  if (!l) return fail("null argument");
  if (l->struct_size != (int)sizeof(rmpc_lidar)) return fail("rmpc_lidar.struct_size mismatch");
  if (B < 1 || l->rays < 1) return fail("lidar project: need B >= 1 and rays >= 1");
  if (l->pose_stride < 3) return fail("lidar project: pose_stride must be >= 3 (x, y, heading)");
  if (l->nbox < 0 || l->ncircle < 0) return fail("lidar project: negative shape count");
  if (!grid_fits(B, l->rays) || !grid_fits(B, l->pose_stride) || !grid_fits(l->nbox, 4) || !grid_fits(l->ncircle, 3))
    return fail("lidar project: B*rays, B*pose_stride, nbox*4 and ncircle*3 must not exceed INT_MAX");
  if (!(l->range > 0.0) || std::isinf(l->range)) return fail("lidar project: range must be positive and finite");
  if (!l->pose || !l->points || !l->ranges) return fail("null argument");
  if (use_device_of(l->pose)) return -1;
  const int n = B * l->rays;
  const double step = (l->angle_max - l->angle_min) / (double)l->rays;
  hipLaunchKernelGGL(k_lidar_project, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, l->pose, l->pose_stride, B,
                     l->rays, l->angle_min, step, l->offset_x, l->offset_y, l->height, l->ranges, l->points);
  return launch_status();
}

// the fields rmpc_scan_match and rmpc_scan_search share, in the order rmpc_scan_match_device has always checked them
extern "C++" template <class M>
static int scan_lattice_check(const std::string &who, int B, const M *m, int max_n) {
  if (B < 1) return fail(who + ": need B >= 1");
  if (m->rays < 1 || m->rays > RMPC_MATCH_MAX_RAYS)
    return fail(who + ": need 1 <= rays <= RMPC_MATCH_MAX_RAYS = " + std::to_string(RMPC_MATCH_MAX_RAYS));
  if (m->pose_stride < 3) return fail(who + ": pose_stride must be >= 3 (x, y, heading)");
  if (m->min_hits < 1) return fail(who + ": need min_hits >= 1");
  if (!grid_fits((long long)B * m->rays, 3) || !grid_fits(B, m->pose_stride))
    return fail(who + ": B*rays*3 and B*pose_stride must not exceed INT_MAX");
  if (!(m->range > 0.0) || std::isinf(m->range)) return fail(who + ": range must be positive and finite");
  if (edge_table_check(who, m->H, m->W, m->sub, m->cap)) return -1;
  if (!grid_fits(m->rays, m->cap)) return fail(who + ": rays*cap must not exceed INT_MAX");
  if (!(m->cell > 0.0) || std::isinf(m->cell) || !std::isfinite(m->x0) || !std::isfinite(m->y0))
    return fail(who + ": cell must be positive and finite, x0 and y0 finite");
  if (m->nxy < 0 || m->nxy > max_n || m->nth < 0 || m->nth > max_n)
    return fail(who + ": nxy and nth must lie in [0, " + std::to_string(max_n) + "]");
  if (!(m->step_xy >= 0.0) || std::isinf(m->step_xy) || !(m->step_th >= 0.0) || std::isinf(m->step_th))
    return fail(who + ": step_xy and step_th must be finite and >= 0");
  if ((m->nxy > 0 && m->step_xy == 0.0) || (m->nth > 0 && m->step_th == 0.0))
    return fail(who + ": a step of 0 needs nxy or nth of 0");
  if (!m->pose || !m->points || !m->ranges || !m->d2 || !m->rot || !m->pose_out || !m->best || !m->score)
    return fail("null argument");
  return 0;
}

int rmpc_scan_match_device(int B, const rmpc_scan_match *m, void *stream) {
  if (!m) return fail("null argument");
  if (m->struct_size != (int)sizeof(rmpc_scan_match)) return fail("rmpc_scan_match.struct_size mismatch");
  if (scan_lattice_check("scan match", B, m, kMatchMaxN)) return -1;
  if (use_device_of(m->pose)) return -1;
  hipLaunchKernelGGL(k_scan_match, dim3(B), dim3(kMatchThreads), 0, (hipStream_t)stream, *m);
  return launch_status();
}

/* wide-window localisation (rmpc_search.hpp) */
int rmpc_grid_min_pyramid_device(int H, int W, int sub, const int32_t *d_d2, int levels, int32_t *d_pyr, void *stream) {
  if (!d_d2 || !d_pyr) return fail("null argument");
  if (edge_table_check("grid min pyramid", H, W, sub, 1)) return -1;
  if (levels < 1 || levels > kSearchMaxLevels) return fail("grid min pyramid: levels must lie in [1, 12]");
  if (use_device_of(d_d2)) return -1;
  const int FH = H * sub, FW = W * sub, n = FH * FW;                   // <= 2^14 * 64
  for (int l = 0; l < levels; l++) {
    const int *const src = l == 0 ? (const int *)d_d2 : (const int *)d_pyr + (size_t)(l - 1) * n;
    hipLaunchKernelGGL(k_min_pyramid, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, src,
                       (int *)d_pyr + (size_t)l * n, FH, FW, l == 0 ? 0 : 1 << (l - 1));
  }
  return launch_status();
}

// the top-level nodes of one robot (include/rmpc.h), 0 on arguments out of range
static long long search_top_nodes(int nxy, int nth, int top_log2) {
  if (nxy < 0 || nxy > kSearchMaxN || nth < 0 || nth > kSearchMaxN || top_log2 < 0 || top_log2 > kSearchMaxTop) return 0;
  const long long nb = ((2 * nxy + 1) + (1 << top_log2) - 1) >> top_log2;
  return (2 * nth + 1) * nb * nb;                                     // <= 255^3
}

int64_t rmpc_scan_search_work_bytes(int B, int nxy, int nth, int top_log2) {
  const long long ntop = search_top_nodes(nxy, nth, top_log2);
  if (B < 1 || ntop == 0) {
    fail("scan search work bytes: need B >= 1, nxy and nth in [0, 127], top_log2 in [0, 7]");
    return -1;
  }
  return (int64_t)B * ntop * (int64_t)sizeof(int32_t);
}

int rmpc_scan_search_device(int B, const rmpc_scan_search *s, void *stream) {
  const std::string who = "scan search";
  if (!s) return fail("null argument");
  if (s->struct_size != (int)sizeof(rmpc_scan_search)) return fail("rmpc_scan_search.struct_size mismatch");
  if (scan_lattice_check(who, B, s, kSearchMaxN)) return -1;
  if (s->top_log2 < 0 || s->top_log2 > kSearchMaxTop) return fail(who + ": top_log2 must lie in [0, 7]");
  if (s->levels < 1 || s->levels > kSearchMaxLevels) return fail(who + ": levels must lie in [1, 12]");
  if (!s->pyr || !s->work) return fail("null argument");
  const long long ntop = search_top_nodes(s->nxy, s->nth, s->top_log2);
  if (!grid_fits(B, ntop)) return fail(who + ": B*ntop must not exceed INT_MAX");
  if (s->work_bytes < rmpc_scan_search_work_bytes(B, s->nxy, s->nth, s->top_log2))
    return fail(who + ": work_bytes is below rmpc_scan_search_work_bytes");
  if (use_device_of(s->pose)) return -1;
  const int nb = ((2 * s->nxy + 1) + (1 << s->top_log2) - 1) >> s->top_log2;
  hipLaunchKernelGGL(k_scan_search, dim3(B), dim3(kSearchThreads), 0, (hipStream_t)stream, *s, (int)ntop, nb);
  return launch_status();
}

/* moving obstacles (rmpc_track.hpp) */
int rmpc_lidar_tracks_device(int B, const rmpc_tracks *t, void *stream) {
  const char *who = "lidar tracks";
  const auto pos = [](double v) { return v > 0.0 && !std::isinf(v); };          // positive and finite
  if (!t) return fail("null argument");
  if (t->struct_size != (int)sizeof(rmpc_tracks)) return fail("rmpc_tracks.struct_size mismatch");
  if (!t->points || !t->ranges || !t->origin || !t->track || !t->age || !t->miss || !t->obst_dyn) return fail("null argument");
  if (B < 1) return fail(std::string(who) + ": need B >= 1");
  if (t->rays < 1 || t->rays > RMPC_TRACK_MAX_RAYS)
    return fail(std::string(who) + ": need 1 <= rays <= RMPC_TRACK_MAX_RAYS = " + std::to_string(RMPC_TRACK_MAX_RAYS));
  if (t->n_tracks < 1 || t->n_tracks > RMPC_TRACK_MAX_TRACKS)
    return fail(std::string(who) + ": need 1 <= n_tracks <= RMPC_TRACK_MAX_TRACKS = " + std::to_string(RMPC_TRACK_MAX_TRACKS));
  if (t->n_out < 1) return fail(std::string(who) + ": need n_out >= 1");
  if (t->min_rays < 1 || t->confirm < 1 || t->max_miss < 0)
    return fail(std::string(who) + ": need min_rays >= 1, confirm >= 1 and max_miss >= 0");
  if (!pos(t->range) || !pos(t->gap) || !pos(t->radius) || !pos(t->gate) || !pos(t->dt))
    return fail(std::string(who) + ": range, gap, radius, gate and dt must be positive and finite");
  if (!(t->alpha > 0.0 && t->alpha <= 1.0)) return fail(std::string(who) + ": alpha must lie in (0, 1]");
  if (!(t->beta >= 0.0 && t->beta <= 2.0)) return fail(std::string(who) + ": beta must lie in [0, 2]");
  if (!(t->margin >= 0.0) || !(t->max_extent >= 0.0) || !(t->v_max >= 0.0))
    return fail(std::string(who) + ": margin, max_extent and v_max must be >= 0");
  if (!std::isfinite(t->park_x) || !std::isfinite(t->park_y)) return fail(std::string(who) + ": park_x, park_y must be finite");
  if (!grid_fits((long long)B * t->rays, 3) || !grid_fits((long long)B * t->n_tracks, 4) || !grid_fits(B, t->n_out) ||
      !grid_fits((long long)B * t->n_out, 9))
    return fail(std::string(who) + ": B*rays*3, B*n_tracks*4 and B*n_out*9 must not exceed INT_MAX");
  {
    const char *const t0 = (const char *)t->track, *const o0 = (const char *)t->obst_dyn;
    const char *const t1 = t0 + (size_t)B * t->n_tracks * 4 * sizeof(double);
    const char *const o1 = o0 + (size_t)B * t->n_out * 9 * sizeof(double);
    if (o0 < t1 && t0 < o1) return fail(std::string(who) + ": obst_dyn must not overlap track");
  }
  if (use_device_of(t->points)) return -1;
  hipLaunchKernelGGL(k_lidar_tracks, dim3(B), dim3(kTrackThreads), 0, (hipStream_t)stream, *t);
  return launch_status();
}

/* timed routes (rmpc_timed.hpp) */
static int timed_common_check(const std::string &who, int B, int T, int sep2, int lag) {
  if (B < 1 || B > RMPC_TIMED_MAX_ROBOTS)
    return fail(who + ": need 1 <= B <= RMPC_TIMED_MAX_ROBOTS = " + std::to_string(RMPC_TIMED_MAX_ROBOTS));
  if (T < 1 || T > RMPC_TIMED_MAX_T) return fail(who + ": need 1 <= T <= RMPC_TIMED_MAX_T = " + std::to_string(RMPC_TIMED_MAX_T));
  if (sep2 < 1 || sep2 > RMPC_TIMED_MAX_SEP2)
    return fail(who + ": need 1 <= sep2 <= RMPC_TIMED_MAX_SEP2 = " + std::to_string(RMPC_TIMED_MAX_SEP2));
  if (lag < 1 || lag > RMPC_TIMED_MAX_LAG) return fail(who + ": lag must lie in [1, " + std::to_string(RMPC_TIMED_MAX_LAG) + "]");
  return 0;
}

// the bytes of workspace of G orders, with `standing` those of the standing rule behind them; -1 for arguments that
// have none
static int64_t timed_work_bytes(const std::string &who, int H, int W, int T, int G, bool standing) {
  if (grid_cells_check(who, H, W, false)) return -1;
  if (T < 1 || T > RMPC_TIMED_MAX_T || G < 1 || G > RMPC_TIMED_MAX_ORDERS)
    return fail(who + ": need 1 <= T <= RMPC_TIMED_MAX_T and 1 <= G <= RMPC_TIMED_MAX_ORDERS");
  const long long shared = standing ? timed_standing_words(H, W) : 0;
  return ((int64_t)G * timed_order_words(H, W, T) + shared) * (int64_t)sizeof(timed_word);
}

// whether `have` bytes are fewer than `need`, the answer of the entry rmpc_<entry>_work_bytes
static int timed_work_check(const std::string &who, const char *entry, int64_t have, int64_t need) {
  if (need < 0) return -1;
  if (have < need)
    return fail(who + ": the workspace holds " + std::to_string(have) + " bytes, " + std::to_string(need) +
                " are needed (rmpc_" + entry + "_work_bytes)");
  return 0;
}

static TimedGeom timed_geom(int H, int W, int T, int sep2) {
  TimedGeom q;
  q.Wd = (W + 63) / 64;
  q.L = H * q.Wd;
  q.rad = 0;
  while ((q.rad + 1) * (q.rad + 1) < sep2) q.rad++;
  q.per_order = timed_order_words(H, W, T);
  return q;
}

int64_t rmpc_timed_plan_work_bytes(int H, int W, int T, int G) { return timed_work_bytes("timed plan", H, W, T, G, false); }

// the argument checks of rmpc_timed_plan_device but for its workspace; `type`: the struct the caller filled
static int timed_plan_args_check(const rmpc_timed_plan *p, const std::string &who, const char *type) {
  if (p->struct_size != (int)sizeof(rmpc_timed_plan)) return fail(std::string(type) + ".struct_size mismatch");
  if (!p->grid || !p->start_cell || !p->goal_index || !p->fields || !p->goal_cells || !p->orders || !p->work || !p->paths ||
      !p->status || !p->arrive || !p->key || !p->best)
    return fail("null argument");
  if (grid_check(p->H, p->W, p->movement) || grid_cells_check(who, p->H, p->W, false) ||
      timed_common_check(who, p->B, p->T, p->sep2, p->lag) || grid_fields_check(who, p->Gf, p->H, p->W))
    return -1;
  if (p->G < 1 || p->G > RMPC_TIMED_MAX_ORDERS)
    return fail(who + ": need 1 <= G <= RMPC_TIMED_MAX_ORDERS = " + std::to_string(RMPC_TIMED_MAX_ORDERS));
  if (!grid_fits((long long)p->G * p->B, p->T + 1)) return fail(who + ": G*B*(T+1) must not exceed INT_MAX");
  return 0;
}

int rmpc_timed_plan_device(const rmpc_timed_plan *p, void *stream) {
  const char *who = "timed plan";
  if (!p) return fail("null argument");
  if (timed_plan_args_check(p, who, "rmpc_timed_plan")) return -1;
  if (timed_work_check(who, "timed_plan", p->work_bytes, rmpc_timed_plan_work_bytes(p->H, p->W, p->T, p->G))) return -1;
  if (use_device_of(p->grid)) return -1;
  const TimedGeom q = timed_geom(p->H, p->W, p->T, p->sep2);
  timed_launch(k_timed_plan<true>, k_timed_plan<false>, p->G, p->T, q, stream, *p, q, (timed_word *)p->work);
  hipLaunchKernelGGL(k_timed_best, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int64_t *)p->key, p->G, (int *)p->best);
  return launch_status();
}

int rmpc_timed_follow_device(int B, int T, const int32_t *d_paths, const int32_t *d_idx_in, int32_t *d_idx_out,
                             const double *d_pos, int stride, int W, double x0, double y0, double cell, double threshold,
                             int sep2, int lag, double *d_goal, int32_t *d_blocked, void *stream) {
  const char *who = "timed follow";
  if (!d_paths || !d_idx_in || !d_idx_out || !d_pos || !d_goal) return fail("null argument");
  if (d_idx_in == d_idx_out) return fail("timed follow: d_idx_out must not be d_idx_in");
  if (timed_common_check(who, B, T, sep2, lag)) return -1;
  if (stride < 2 || !grid_fits(B, stride) || W < 1) return fail("timed follow: need stride >= 2, W >= 1");
  if (use_device_of(d_paths)) return -1;
  hipLaunchKernelGGL(k_timed_follow, dim3(B), dim3(256), 0, (hipStream_t)stream, (const int *)d_paths, B, T,
                     (const int *)d_idx_in, (int *)d_idx_out, d_pos, stride, W, x0, y0, cell, threshold, sep2, lag, d_goal,
                     (int *)d_blocked);
  return launch_status();
}

/* timed tours (rmpc_timed_tours.hpp, include/rmpc_timed_tours.h) */
int64_t rmpc_timed_tours_work_bytes(int H, int W, int T, int G) { return timed_work_bytes("timed tours", H, W, T, G, false); }

static int timed_tours_stops_check(const std::string &who, int K) {
  if (K < 1 || K > RMPC_TIMED_TOURS_MAX_STOPS)
    return fail(who + ": need 1 <= K <= RMPC_TIMED_TOURS_MAX_STOPS = " + std::to_string(RMPC_TIMED_TOURS_MAX_STOPS));
  return 0;
}

// the argument checks of rmpc_timed_tours_plan_device; own_work: p->work is the call's workspace
static int timed_tours_args_check(const rmpc_timed_tours *p, bool own_work) {
  const char *who = "timed tours";
  if (!p) return fail("null argument");
  if (p->struct_size != (int)sizeof(rmpc_timed_tours)) return fail("rmpc_timed_tours.struct_size mismatch");
  if (!p->grid || !p->start_cell || !p->stops || !p->len || !p->park_index || !p->fields || !p->goal_cells || !p->orders ||
      (own_work && !p->work) || !p->paths || !p->status || !p->arrive || !p->key || !p->best || !p->serve_at || !p->served ||
      !p->unserved)
    return fail("null argument");
  if (grid_check(p->H, p->W, p->movement) || grid_cells_check(who, p->H, p->W, false) ||
      timed_common_check(who, p->B, p->T, p->sep2, p->lag) || grid_fields_check(who, p->Gf, p->H, p->W) ||
      timed_tours_stops_check(who, p->K))
    return -1;
  if (p->dwell < 0 || p->dwell > RMPC_TIMED_TOURS_MAX_DWELL)
    return fail("timed tours: need 0 <= dwell <= RMPC_TIMED_TOURS_MAX_DWELL = " + std::to_string(RMPC_TIMED_TOURS_MAX_DWELL));
  if (p->G < 1 || p->G > RMPC_TIMED_MAX_ORDERS)
    return fail("timed tours: need 1 <= G <= RMPC_TIMED_MAX_ORDERS = " + std::to_string(RMPC_TIMED_MAX_ORDERS));
  if (!grid_fits((long long)p->G * p->B, p->T + 1)) return fail("timed tours: G*B*(T+1) must not exceed INT_MAX");
  if (!grid_fits((long long)p->G * p->B, p->K)) return fail("timed tours: G*B*K must not exceed INT_MAX");
  if (!own_work) return 0;
  return timed_work_check(who, "timed_tours", p->work_bytes, rmpc_timed_tours_work_bytes(p->H, p->W, p->T, p->G));
}

int rmpc_timed_tours_plan_device(const rmpc_timed_tours *p, void *stream) {
  if (timed_tours_args_check(p, true)) return -1;
  if (use_device_of(p->grid)) return -1;
  const TimedGeom q = timed_geom(p->H, p->W, p->T, p->sep2);
  timed_launch(k_timed_tours_plan<true>, k_timed_tours_plan<false>, p->G, p->T, q, stream, *p, q, (timed_word *)p->work);
  hipLaunchKernelGGL(k_timed_tours_best, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int64_t *)p->key,
                     (const int *)p->unserved, p->G, (int *)p->best);
  return launch_status();
}

int rmpc_timed_tours_follow_device(int B, int T, const int32_t *d_paths, const int32_t *d_idx_in, int32_t *d_idx_out,
                                   const double *d_pos, int stride, int W, double x0, double y0, double cell,
                                   double threshold, int sep2, int lag, double *d_goal, int32_t *d_blocked, int K,
                                   const int32_t *d_serve_at, int32_t *d_leg, int32_t *d_served, int now, double stop_tol,
                                   void *stream) {
  const char *who = "timed tours follow";
  if (!d_paths || !d_idx_in || !d_idx_out || !d_pos || !d_goal || !d_serve_at || !d_leg || !d_served)
    return fail("null argument");
  if (d_idx_in == d_idx_out) return fail("timed tours follow: d_idx_out must not be d_idx_in");
  if (timed_common_check(who, B, T, sep2, lag) || timed_tours_stops_check(who, K)) return -1;
  if (stride < 2 || !grid_fits(B, stride) || W < 1) return fail("timed tours follow: need stride >= 2, W >= 1");
  if (!(stop_tol >= 0.0)) return fail("timed tours follow: stop_tol must be >= 0");
  if (use_device_of(d_paths)) return -1;
  hipLaunchKernelGGL(k_timed_tours_follow, dim3(B), dim3(256), 0, (hipStream_t)stream, (const int *)d_paths, B, T,
                     (const int *)d_idx_in, (int *)d_idx_out, d_pos, stride, W, x0, y0, cell, threshold, sep2, lag, d_goal,
                     (int *)d_blocked, K, (const int *)d_serve_at, (int *)d_leg, (int *)d_served, now, stop_tol);
  return launch_status();
}

/* lifelong timed tours (rmpc_timed_replan.hpp, include/rmpc_timed_replan.h) */
int64_t rmpc_timed_reserve_words(int H, int W, int T) {
  if (grid_cells_check("timed reserve", H, W, false)) return -1;
  if (T < 1 || T > RMPC_TIMED_MAX_T) return fail("timed reserve: need 1 <= T <= RMPC_TIMED_MAX_T");
  return (int64_t)(T + 1) * H * ((W + 63) / 64);
}

int rmpc_timed_reserve_device(int H, int W, int T, int P, const int32_t *d_cells, const int32_t *d_use, int sep2, int lag,
                              int clear, uint64_t *d_res, void *stream) {
  const char *who = "timed reserve";
  if (!d_cells || !d_res) return fail("null argument");
  if (grid_cells_check(who, H, W, false) || timed_common_check(who, 1, T, sep2, lag)) return -1;
  if (P < 1 || P > RMPC_TIMED_RESERVE_MAX_PATHS)
    return fail("timed reserve: need 1 <= P <= RMPC_TIMED_RESERVE_MAX_PATHS = " + std::to_string(RMPC_TIMED_RESERVE_MAX_PATHS));
  if (use_device_of(d_res)) return -1;
  const TimedGeom q = timed_geom(H, W, T, sep2);
  if (clear) {
    const hipError_t e = hipMemsetAsync(d_res, 0, (size_t)(T + 1) * q.L * sizeof(timed_word), (hipStream_t)stream);
    if (e != hipSuccess) return fail(std::string("timed reserve: hipMemsetAsync: ") + hipGetErrorString(e));
  }
  hipLaunchKernelGGL(k_timed_reserve, dim3(P), dim3(kTimedThreads), 0, (hipStream_t)stream, H, W, T, (const int *)d_cells,
                     (const int *)d_use, sep2, lag, q.rad, q.Wd, q.L, (timed_word *)d_res);
  return launch_status();
}

int64_t rmpc_timed_replan_work_bytes(int H, int W, int T, int G) {
  return timed_work_bytes("timed replan", H, W, T, G, true);
}

int rmpc_timed_tours_replan_device(const rmpc_timed_tours *p, const rmpc_timed_replan *x, void *stream) {
  if (!x) return fail("null argument");
  if (x->struct_size != (int)sizeof(rmpc_timed_replan)) return fail("rmpc_timed_replan.struct_size mismatch");
  if (timed_tours_args_check(p, false)) return -1;
  if (!x->work) return fail("null argument");
  if (timed_work_check("timed replan", "timed_replan", x->work_bytes, rmpc_timed_replan_work_bytes(p->H, p->W, p->T, p->G)))
    return -1;
  if (use_device_of(p->grid)) return -1;
  const TimedGeom q = timed_geom(p->H, p->W, p->T, p->sep2);
  timed_word *const work = (timed_word *)x->work;
  hipLaunchKernelGGL(k_timed_standing, dim3((p->H * p->W + 255) / 256), dim3(256), 0, (hipStream_t)stream, *p, *x, q.Wd, q.L,
                     work + (size_t)p->G * q.per_order);
  timed_launch(k_timed_tours_replan<true>, k_timed_tours_replan<false>, p->G, p->T, q, stream, *p, *x, q, work);
  hipLaunchKernelGGL(k_timed_tours_best, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int64_t *)p->key,
                     (const int *)p->unserved, p->G, (int *)p->best);
  return launch_status();
}

/* timed routes with repaired orders (rmpc_timed_repair.hpp, include/rmpc_timed_repair.h) */
int64_t rmpc_timed_plan_repair_work_bytes(int H, int W, int T, int G, int B) {
  const char *who = "timed repair";
  const int64_t plan = timed_work_bytes(who, H, W, T, G, false);
  if (plan < 0) return -1;
  if (B < 1 || B > RMPC_TIMED_MAX_ROBOTS)
    return fail(std::string(who) + ": need 1 <= B <= RMPC_TIMED_MAX_ROBOTS = " + std::to_string(RMPC_TIMED_MAX_ROBOTS));
  return plan + (int64_t)G * timed_repair_words(T, B) * (int64_t)sizeof(timed_word);
}

int rmpc_timed_plan_repair_device(const rmpc_timed_repair *x, void *stream) {
  const char *who = "timed repair";
  if (!x) return fail("null argument");
  if (x->struct_size != (int)sizeof(rmpc_timed_repair)) return fail("rmpc_timed_repair.struct_size mismatch");
  // the members up to `best` are rmpc_timed_plan's: the plan's own checks and kernels' parts take them as such
  rmpc_timed_plan p;
  p.struct_size = (int32_t)sizeof(rmpc_timed_plan);
  p.H = x->H; p.W = x->W; p.movement = x->movement;
  p.grid = x->grid; p.occ_threshold = x->occ_threshold;
  p.B = x->B; p.Gf = x->Gf;
  p.start_cell = x->start_cell; p.goal_index = x->goal_index; p.fields = x->fields; p.goal_cells = x->goal_cells;
  p.T = x->T; p.sep2 = x->sep2; p.lag = x->lag; p.G = x->G;
  p.orders = x->orders;
  p.work = x->work; p.work_bytes = x->work_bytes;
  p.paths = x->paths; p.status = x->status; p.arrive = x->arrive; p.key = x->key; p.best = x->best;
  if (!x->order_out || !x->rounds_run || !x->round_best) return fail("null argument");
  if (timed_plan_args_check(&p, who, "rmpc_timed_repair")) return -1;
  if (x->rounds < 0 || x->rounds > RMPC_TIMED_MAX_ROUNDS)
    return fail(std::string(who) + ": need 0 <= rounds <= RMPC_TIMED_MAX_ROUNDS = " + std::to_string(RMPC_TIMED_MAX_ROUNDS));
  if (timed_work_check(who, "timed_plan_repair", p.work_bytes, rmpc_timed_plan_repair_work_bytes(p.H, p.W, p.T, p.G, p.B)))
    return -1;
  if (use_device_of(p.grid)) return -1;
  const TimedGeom q = timed_geom(p.H, p.W, p.T, p.sep2);
  const TimedRepair rep = {x->rounds, (int *)x->order_out, (int *)x->rounds_run, (int *)x->round_best};
  timed_launch(k_timed_plan_repair<true>, k_timed_plan_repair<false>, p.G, p.T, q, stream, p, rep, q, (timed_word *)p.work);
  hipLaunchKernelGGL(k_timed_best, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int64_t *)p.key, p.G, (int *)p.best);
  return launch_status();
}

/* optimal timed routes: conflict-based search (rmpc_cbs.hpp, include/rmpc_cbs.h): every refusal comes
 * before the first HIP call */
static int cbs_sizes_check(const std::string &who, int H, int W, int T, int B, int nodes, int expand) {
  if (grid_cells_check(who, H, W, false)) return -1;
  if (T < 1 || T > RMPC_TIMED_MAX_T) return fail(who + ": need 1 <= T <= RMPC_TIMED_MAX_T = " + std::to_string(RMPC_TIMED_MAX_T));
  if (B < 1 || B > RMPC_CBS_MAX_ROBOTS)
    return fail(who + ": need 1 <= B <= RMPC_CBS_MAX_ROBOTS = " + std::to_string(RMPC_CBS_MAX_ROBOTS));
  if (nodes < 1 || nodes > RMPC_CBS_MAX_NODES)
    return fail(who + ": need 1 <= nodes <= RMPC_CBS_MAX_NODES = " + std::to_string(RMPC_CBS_MAX_NODES));
  if (expand < 1 || expand > RMPC_CBS_MAX_EXPAND)
    return fail(who + ": need 1 <= expand <= RMPC_CBS_MAX_EXPAND = " + std::to_string(RMPC_CBS_MAX_EXPAND));
  return 0;
}

int64_t rmpc_cbs_work_bytes(int H, int W, int T, int B, int nodes, int expand) {
  if (cbs_sizes_check("cbs", H, W, T, B, nodes, expand)) return -1;
  return cbs_layout(H, W, T, B, nodes, expand).total;
}

// what names a search in its workspace: a resumed call must bring the sizes and rules the search was started with
static int cbs_magic(const rmpc_cbs *p) {
  uint32_t m = 0x43425331u;
  for (int v : {p->H, p->W, p->movement, p->B, p->Gf, p->T, p->sep2, p->lag, p->nodes, p->expand}) m = (m ^ (uint32_t)v) * 16777619u;
  return (int)(m | 1u);
}

int rmpc_cbs_device(const rmpc_cbs *p, void *stream) {
  const std::string who = "cbs";
  if (!p) return fail("null argument");
  if (p->struct_size != (int)sizeof(rmpc_cbs)) return fail("rmpc_cbs.struct_size mismatch");
  if (!p->grid || !p->start_cell || !p->goal_index || !p->fields || !p->goal_cells || !p->work || !p->paths || !p->status ||
      !p->arrive || !p->info)
    return fail("null argument");
  if (grid_check(p->H, p->W, p->movement) || cbs_sizes_check(who, p->H, p->W, p->T, p->B, p->nodes, p->expand) ||
      timed_common_check(who, p->B, p->T, p->sep2, p->lag) || grid_fields_check(who, p->Gf, p->H, p->W))
    return -1;
  if (p->rounds < 0 || p->rounds > RMPC_CBS_MAX_ROUNDS)
    return fail(who + ": need 0 <= rounds <= RMPC_CBS_MAX_ROUNDS = " + std::to_string(RMPC_CBS_MAX_ROUNDS));
  if (timed_work_check(who, "cbs", p->work_bytes, rmpc_cbs_work_bytes(p->H, p->W, p->T, p->B, p->nodes, p->expand))) return -1;
  if (use_device_of(p->grid)) return -1;
  TimedGeom q = timed_geom(p->H, p->W, p->T, p->sep2);
  const CbsLayout y = cbs_layout(p->H, p->W, p->T, p->B, p->nodes, p->expand);
  q.per_order = y.slot_words;
  const int magic = cbs_magic(p);
  if (!p->resume) timed_launch(k_cbs_root<true>, k_cbs_root<false>, 1, p->T, q, stream, *p, q, y, magic);
  for (int r = 0; r < p->rounds; r++) {
    hipLaunchKernelGGL(k_cbs_select, dim3(1), dim3(256), 0, (hipStream_t)stream, *p, y, magic, r == 0, 0);
    timed_launch(k_cbs_expand<true>, k_cbs_expand<false>, 2 * p->expand, p->T, q, stream, *p, q, y);
  }
  hipLaunchKernelGGL(k_cbs_select, dim3(1), dim3(256), 0, (hipStream_t)stream, *p, y, magic, p->rounds == 0, 1);
  return launch_status();
}

/* bounded-suboptimal timed routes: focal conflict-based search (rmpc_ecbs.hpp, include/rmpc_ecbs.h): every
 * refusal comes before the first HIP call */
int64_t rmpc_ecbs_work_bytes(int H, int W, int T, int B, int nodes, int expand) {
  if (cbs_sizes_check("ecbs", H, W, T, B, nodes, expand)) return -1;
  return ecbs_layout(H, W, T, B, nodes, expand).total;
}

static int ecbs_magic(const rmpc_ecbs *p) {
  uint32_t m = 0x45434253u;
  for (int v : {p->H, p->W, p->movement, p->B, p->Gf, p->T, p->sep2, p->lag, p->nodes, p->expand, p->w_num, p->w_den})
    m = (m ^ (uint32_t)v) * 16777619u;
  return (int)(m | 1u);
}

int rmpc_ecbs_device(const rmpc_ecbs *p, void *stream) {
  const std::string who = "ecbs";
  if (!p) return fail("null argument");
  if (p->struct_size != (int)sizeof(rmpc_ecbs)) return fail("rmpc_ecbs.struct_size mismatch");
  if (!p->grid || !p->start_cell || !p->goal_index || !p->fields || !p->goal_cells || !p->work || !p->paths || !p->status ||
      !p->arrive || !p->info)
    return fail("null argument");
  if (grid_check(p->H, p->W, p->movement) || cbs_sizes_check(who, p->H, p->W, p->T, p->B, p->nodes, p->expand) ||
      timed_common_check(who, p->B, p->T, p->sep2, p->lag) || grid_fields_check(who, p->Gf, p->H, p->W))
    return -1;
  if (p->rounds < 0 || p->rounds > RMPC_CBS_MAX_ROUNDS)
    return fail(who + ": need 0 <= rounds <= RMPC_CBS_MAX_ROUNDS = " + std::to_string(RMPC_CBS_MAX_ROUNDS));
  if (p->w_den < 1 || p->w_den > RMPC_ECBS_MAX_W_DEN)
    return fail(who + ": need 1 <= w_den <= RMPC_ECBS_MAX_W_DEN = " + std::to_string(RMPC_ECBS_MAX_W_DEN));
  if (p->w_num < p->w_den || (long long)p->w_num > (long long)RMPC_ECBS_MAX_W * p->w_den)
    return fail(who + ": need w_den <= w_num <= RMPC_ECBS_MAX_W * w_den, RMPC_ECBS_MAX_W = " + std::to_string(RMPC_ECBS_MAX_W));
  if (timed_work_check(who, "ecbs", p->work_bytes, rmpc_ecbs_work_bytes(p->H, p->W, p->T, p->B, p->nodes, p->expand))) return -1;
  if (use_device_of(p->grid)) return -1;
  TimedGeom q = timed_geom(p->H, p->W, p->T, p->sep2);
  const EcbsLayout y = ecbs_layout(p->H, p->W, p->T, p->B, p->nodes, p->expand);
  q.per_order = y.slot_words;
  const int magic = ecbs_magic(p);
  if (!p->resume)
    ecbs_launch(k_ecbs_root<true, true>, k_ecbs_root<true, false>, k_ecbs_root<false, true>, k_ecbs_root<false, false>, 1, p->H, p->W,
                p->T, q, stream, *p, q, y, magic);
  for (int r = 0; r < p->rounds; r++) {
    hipLaunchKernelGGL(k_ecbs_select, dim3(1), dim3(256), 0, (hipStream_t)stream, *p, y, magic, r == 0, 0);
    ecbs_launch(k_ecbs_expand<true, true>, k_ecbs_expand<true, false>, k_ecbs_expand<false, true>, k_ecbs_expand<false, false>,
                2 * p->expand, p->H, p->W, p->T, q, stream, *p, q, y);
  }
  hipLaunchKernelGGL(k_ecbs_select, dim3(1), dim3(256), 0, (hipStream_t)stream, *p, y, magic, p->rounds == 0, 1);
  return launch_status();
}

/* line of sight, shortened routes and the follower that looks ahead (rmpc_any_angle.hpp, include/rmpc_any_angle.h,
 * DESIGN.md 28): every refusal comes before the first HIP call */
static int any_angle_map_check(const std::string &who, int H, int W) {
  if (H < 1 || W < 1) return fail(who + ": need H, W >= 1");
  if ((long long)H * W > RMPC_GRID_LARGE_MAX_CELLS)
    return fail(who + ": " + std::to_string(H) + "x" + std::to_string(W) + " map exceeds RMPC_GRID_LARGE_MAX_CELLS = " +
                std::to_string(RMPC_GRID_LARGE_MAX_CELLS) + " cells");
  return 0;
}

int rmpc_grid_visible_device(int H, int W, const double *d_grid, double occ_threshold, int P, const int32_t *d_from,
                             const int32_t *d_to, int32_t *d_visible, void *stream) {
  const std::string who = "grid visible";
  if (!d_grid || !d_from || !d_to || !d_visible) return fail("null argument");
  if (any_angle_map_check(who, H, W)) return -1;
  if (P < 1) return fail(who + ": need P >= 1");
  if (use_device_of(d_grid)) return -1;
  hipLaunchKernelGGL(k_grid_visible, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_grid, H, W, occ_threshold,
                     P, (const int *)d_from, (const int *)d_to, (int *)d_visible);
  return launch_status();
}

int rmpc_grid_shorten_device(int H, int W, const double *d_grid, double occ_threshold, int B, const int32_t *d_path,
                             const int32_t *d_len, int max_len, int reach, const int32_t *d_keep, int32_t *d_out,
                             int32_t *d_out_len, int32_t *d_src, void *d_work, void *stream) {
  const std::string who = "grid shorten";
  if (!d_grid || !d_path || !d_len || !d_out || !d_out_len || !d_work) return fail("null argument");
  if (any_angle_map_check(who, H, W) || grid_paths_check(who, B, max_len)) return -1;
  if (reach < 0) return fail(who + ": reach must be >= 0 (0: the whole path)");
  if (d_out == d_path) return fail(who + ": d_out may not be d_path");
  if (use_device_of(d_grid)) return -1;
  const bool lds = max_len <= kShortenLdsCells;
#ifdef RMPC_SHORTEN_READS_GRID      // the measurement of DESIGN.md 28: no bit image, the walks read the doubles
  const OccGrid occ{d_grid, W, occ_threshold};
#else
  const int waves = H * ((W + 63) / 64);
  hipLaunchKernelGGL(k_grid_occ_bits, dim3((waves + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_grid, H, W, occ_threshold,
                     (unsigned *)d_work);
  const OccBits occ{(const unsigned *)d_work, (W + 31) / 32};
#endif
  auto kernel = lds ? k_grid_shorten<true, decltype(occ)> : k_grid_shorten<false, decltype(occ)>;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(64), lds ? (size_t)max_len * sizeof(int) : 0, (hipStream_t)stream, occ, H, W, B,
                     (const int *)d_path, (const int *)d_len, max_len, reach, (const int *)d_keep, (int *)d_out,
                     (int *)d_out_len, (int *)d_src);
  return launch_status();
}

int rmpc_follow_visible_device(int B, const int32_t *d_path, const int32_t *d_len, int max_len, int32_t *d_idx,
                               const double *d_pos, int stride, int H, int W, const double *d_grid, double occ_threshold,
                               double x0, double y0, double cell, int reach, double look_ahead, double *d_goal,
                               int32_t *d_blocked, void *stream) {
  const std::string who = "follow visible";
  if (!d_path || !d_len || !d_idx || !d_pos || !d_grid || !d_goal) return fail("null argument");
  if (grid_paths_check(who, B, max_len) || any_angle_map_check(who, H, W)) return -1;
  if (stride < 2 || !grid_fits(B, stride)) return fail(who + ": need stride >= 2 and B*stride <= INT_MAX");
  if (reach < 1 || reach > RMPC_VISIBLE_MAX_REACH)
    return fail(who + ": need 1 <= reach <= RMPC_VISIBLE_MAX_REACH = " + std::to_string(RMPC_VISIBLE_MAX_REACH));
  if (!(cell > 0.0) || std::isinf(cell)) return fail(who + ": cell must be finite and > 0");
  if (!(look_ahead > 0.0) || std::isinf(look_ahead) || look_ahead < 2.0 * cell)
    return fail(who + ": look_ahead must be finite and >= 2 cell");
  if (use_device_of(d_path)) return -1;
  hipLaunchKernelGGL(k_follow_visible, dim3((B + kFollowWaves - 1) / kFollowWaves), dim3(64 * kFollowWaves), 0,
                     (hipStream_t)stream, (const int *)d_path, (const int *)d_len, max_len, (int *)d_idx, d_pos, stride, B, H,
                     W, d_grid, occ_threshold, x0, y0, cell, reach, look_ahead, d_goal, (int *)d_blocked);
  return launch_status();
}

/* safe corridors from the map (rmpc_corridor.hpp, include/rmpc_corridor.h): every refusal comes before
 * the first HIP call */
int rmpc_grid_occ_sums_device(int H, int W, const double *d_grid, double occ_threshold, int32_t *d_sums, void *stream) {
  const std::string who = "grid occ sums";
  if (!d_grid || !d_sums) return fail("null argument");
  if (any_angle_map_check(who, H, W)) return -1;
  if (!std::isfinite(occ_threshold)) return fail(who + ": occ_threshold must be finite");
  if (use_device_of(d_grid)) return -1;
  hipLaunchKernelGGL(k_occ_row_sums, dim3((H + kSumsRowWaves - 1) / kSumsRowWaves), dim3(64 * kSumsRowWaves), 0,
                     (hipStream_t)stream, d_grid, H, W, occ_threshold, (int *)d_sums);
  hipLaunchKernelGGL(k_occ_col_sums, dim3((W + 1 + 255) / 256), dim3(256), 0, (hipStream_t)stream, H, W, (int *)d_sums);
  return launch_status();
}

int rmpc_grid_corridor_device(int H, int W, const int32_t *d_sums, double x0, double y0, double cell, int B, int N,
                              const double *d_points, int reach, int nobst, int slot0, double *d_planes, int32_t *d_rect,
                              int32_t *d_status, void *stream) {
  const std::string who = "grid corridor";
  if (!d_sums || !d_points || !d_planes) return fail("null argument");
  if (any_angle_map_check(who, H, W)) return -1;
  if (B < 1 || N < 1) return fail(who + ": need B, N >= 1");
  if (reach < 1 || reach > RMPC_CORRIDOR_MAX_REACH)
    return fail(who + ": need 1 <= reach <= RMPC_CORRIDOR_MAX_REACH = " + std::to_string(RMPC_CORRIDOR_MAX_REACH));
  if (slot0 < 0 || nobst < 4 || slot0 > nobst - 4) return fail(who + ": need 0 <= slot0 and slot0 + 4 <= nobst");
  if (!grid_fits(B, N) || !grid_fits((long long)B * N, nobst) || !grid_fits((long long)B * N * nobst, 4))
    return fail(who + ": B*N*nobst*4 must not exceed INT_MAX");
  if (!(cell > 0.0) || std::isinf(cell)) return fail(who + ": cell must be finite and > 0");
  if (!std::isfinite(x0) || !std::isfinite(y0)) return fail(who + ": x0 and y0 must be finite");
  if (use_device_of(d_sums)) return -1;
  const int n = B * N;
  hipLaunchKernelGGL(k_grid_corridor, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const int *)d_sums, H, W, x0,
                     y0, cell, n, d_points, reach, nobst, slot0, d_planes, (int *)d_rect, (int *)d_status);
  return launch_status();
}

/* traffic-aware routes (rmpc_traffic.hpp, include/rmpc_traffic.h): every refusal comes before the first
 * HIP call */
static int traffic_map_check(const std::string &who, int H, int W) {
  if (H < 1 || W < 1) return fail(who + ": need H, W >= 1");
  if ((long long)H * W > RMPC_GRID_MAX_CELLS)
    return fail(who + ": " + std::to_string(H) + "x" + std::to_string(W) + " map exceeds RMPC_GRID_MAX_CELLS = " +
                std::to_string(RMPC_GRID_MAX_CELLS) + " cells");
  return 0;
}
static int traffic_costs_check(const std::string &who, const rmpc_traffic_costs *c, TrafficCosts *out) {
  if (c->struct_size != (int)sizeof(rmpc_traffic_costs)) return fail("rmpc_traffic_costs.struct_size mismatch");
  if (c->base_axial < 1 || c->base_diag < 1) return fail(who + ": base_axial and base_diag must be >= 1");
  if (c->w_visit < 0 || c->w_contra < 0 || c->cap_visit < 0 || c->cap_contra < 0)
    return fail(who + ": weights and caps must be >= 0");
  if (c->cap_visit > RMPC_TRAFFIC_MAX_CAP_VISIT)
    return fail(who + ": cap_visit exceeds RMPC_TRAFFIC_MAX_CAP_VISIT = " + std::to_string(RMPC_TRAFFIC_MAX_CAP_VISIT));
  if (c->cap_contra > RMPC_TRAFFIC_MAX_CAP_CONTRA)
    return fail(who + ": cap_contra exceeds RMPC_TRAFFIC_MAX_CAP_CONTRA = " + std::to_string(RMPC_TRAFFIC_MAX_CAP_CONTRA));
  const long long edge = (long long)(c->base_axial > c->base_diag ? c->base_axial : c->base_diag) +
                         (long long)c->w_visit * c->cap_visit + (long long)c->w_contra * c->cap_contra;
  if (edge > RMPC_TRAFFIC_MAX_EDGE)
    return fail(who + ": the largest edge cost " + std::to_string(edge) + " exceeds RMPC_TRAFFIC_MAX_EDGE = " +
                std::to_string(RMPC_TRAFFIC_MAX_EDGE));
  *out = TrafficCosts{c->base_axial, c->base_diag, c->w_visit, c->cap_visit, c->w_contra, c->cap_contra};
  return 0;
}
static int traffic_movement_check(const std::string &who, int movement) {
  return movement != 4 && movement != 8 ? fail(who + ": movement must be 4 or 8") : 0;
}

int rmpc_grid_traffic_add_device(int H, int W, int B, const int32_t *d_path, const int32_t *d_len, int max_len,
                                 const int32_t *d_select, int sign, int32_t *d_flow, void *stream) {
  const std::string who = "grid traffic add";
  if (!d_path || !d_len || !d_flow) return fail("null argument");
  if (traffic_map_check(who, H, W) || grid_paths_check(who, B, max_len)) return -1;
  if (sign != 1 && sign != -1) return fail(who + ": sign must be +1 or -1");
  if (use_device_of(d_path)) return -1;
  const long long n = (long long)B * max_len;
  hipLaunchKernelGGL(k_traffic_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, H, W, B,
                     (const int *)d_path, (const int *)d_len, max_len, (const int *)d_select, sign, (int *)d_flow);
  return launch_status();
}

int rmpc_grid_fields_traffic_device(int H, int W, const double *d_grid, double occ_threshold, const int32_t *d_flow,
                                    const rmpc_traffic_costs *costs, int G, const int32_t *d_goal_cells, int movement,
                                    int32_t *d_fields, int32_t *d_status, int32_t *d_sweeps, void *stream) {
  const std::string who = "grid fields traffic";
  TrafficCosts k;
  if (!d_grid || !d_flow || !costs || !d_goal_cells || !d_fields || !d_status) return fail("null argument");
  if (traffic_map_check(who, H, W) || traffic_movement_check(who, movement) || grid_fields_check(who, G, H, W)) return -1;
  if (std::isnan(occ_threshold)) return fail(who + ": occ_threshold must not be a NaN");
  if (traffic_costs_check(who, costs, &k) || use_device_of(d_grid)) return -1;
  hipLaunchKernelGGL(k_traffic_fields, dim3(G), dim3(kGridThreads), 0, (hipStream_t)stream, d_grid, H, W, occ_threshold,
                     (const int *)d_flow, k, (const int *)d_goal_cells, movement, (int *)d_fields, (int *)d_status,
                     (int *)d_sweeps);
  return launch_status();
}

int rmpc_grid_paths_traffic_device(int H, int W, const double *d_grid, double occ_threshold, const int32_t *d_flow,
                                   const rmpc_traffic_costs *costs, int G, const int32_t *d_fields,
                                   const int32_t *d_goal_cells, int B, const int32_t *d_start_cell,
                                   const int32_t *d_goal_index, int movement, int max_len, int32_t *d_path, int32_t *d_len,
                                   void *stream) {
  const std::string who = "grid paths traffic";
  TrafficCosts k;
  if (!d_grid || !d_flow || !costs || !d_fields || !d_goal_cells || !d_start_cell || !d_goal_index || !d_path || !d_len)
    return fail("null argument");
  if (traffic_map_check(who, H, W) || traffic_movement_check(who, movement) || grid_fields_check(who, G, H, W) ||
      grid_paths_check(who, B, max_len))
    return -1;
  if (std::isnan(occ_threshold)) return fail(who + ": occ_threshold must not be a NaN");
  if (traffic_costs_check(who, costs, &k) || use_device_of(d_grid)) return -1;
  hipLaunchKernelGGL(k_traffic_paths, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_grid, H, W, occ_threshold,
                     (const int *)d_flow, k, (const int *)d_fields, (const int *)d_goal_cells, G, (const int *)d_start_cell,
                     (const int *)d_goal_index, B, movement, max_len, (int *)d_path, (int *)d_len);
  return launch_status();
}

int rmpc_grid_traffic_score_device(int H, int W, const int32_t *d_flow, int base_axial, int base_diag, int64_t *d_score,
                                   void *stream) {
  const std::string who = "grid traffic score";
  if (!d_flow || !d_score) return fail("null argument");
  if (traffic_map_check(who, H, W)) return -1;
  if (base_axial < 1 || base_diag < 1) return fail(who + ": base_axial and base_diag must be >= 1");
  if (use_device_of(d_flow)) return -1;
  hipLaunchKernelGGL(k_traffic_score, dim3(1), dim3(kTrafficScoreThreads), 0, (hipStream_t)stream, H, W, (const int *)d_flow,
                     base_axial, base_diag, (long long *)d_score);
  return launch_status();
}

}  // extern "C"
