// The host side of the timed tours under AddressSanitizer + UBSan, as a program of its own: the argument checks of
// rmpc_timed_tours_plan_device and rmpc_timed_tours_follow_device and the work-size query (rmpc_world.hip) are plain C++
// that runs before any HIP call.  Every call below is refused (-1 with the entry's message); the pointers are never read.
//   bash tests/host/run_refusals.sh timed_tours
#include "../../robot_mpcs_amd/csrc/rmpc_world.hip"

#include <cmath>
#include <cstdio>

static int g_bad = 0;
static void refused(long long rc, const char *want, const char *what) {
  if (rc != -1 || g_err.find(want) == std::string::npos) {
    std::printf("NOT REFUSED %s: rc %lld, message '%s'\n", what, rc, g_err.c_str());
    g_bad++;
  }
}

struct FollowArgs {
  int B = 2, T = 5, stride = 3, W = 41, sep2 = 9, lag = 1, K = 2, now = 0;
  const int32_t *paths, *idx_in, *serve_at;
  int32_t *idx_out, *leg, *served;
  const double *pos;
  double *goal;
  double stop_tol = 0.2;
};
static long long follow(const FollowArgs &a) {
  return rmpc_timed_tours_follow_device(a.B, a.T, a.paths, a.idx_in, a.idx_out, a.pos, a.stride, a.W, 0.0, 0.0, 0.5, 1.3, a.sep2,
                                        a.lag, a.goal, nullptr, a.K, a.serve_at, a.leg, a.served, a.now, a.stop_tol, nullptr);
}

int main() {
  static double buf[64];
  rmpc_timed_tours t = {};
  t.struct_size = (int32_t)sizeof(rmpc_timed_tours);
  t.H = 7; t.W = 5; t.movement = 4;
  t.grid = t.fields = buf;
  t.occ_threshold = 0.8;
  t.B = 3; t.Gf = 2; t.K = 2; t.dwell = 1;
  t.start_cell = t.stops = t.len = t.park_index = t.goal_cells = t.orders = (const int32_t *)buf;
  t.T = 9; t.sep2 = 2; t.lag = 1; t.G = 2;
  t.work = buf; t.work_bytes = 1 << 20;
  t.paths = t.status = t.arrive = t.best = t.serve_at = t.served = t.unserved = (int32_t *)buf;
  t.key = (int64_t *)buf;
  const int64_t full = rmpc_timed_tours_work_bytes(7, 5, 9, 2);
  if (full != rmpc_timed_plan_work_bytes(7, 5, 9, 2) || full != 2 * 8 * (2 * 10 * 7 + 2 * 7 + 18)) {
    std::printf("work bytes %lld\n", (long long)full);
    g_bad++;
  }
#define TRY(field, value, want)                                              \
  {                                                                          \
    rmpc_timed_tours a = t;                                                  \
    a.field = value;                                                         \
    refused(rmpc_timed_tours_plan_device(&a, nullptr), want, #field " = " #value); \
  }
  TRY(grid, nullptr, "null argument") TRY(start_cell, nullptr, "null argument") TRY(stops, nullptr, "null argument")
  TRY(len, nullptr, "null argument") TRY(park_index, nullptr, "null argument") TRY(fields, nullptr, "null argument")
  TRY(goal_cells, nullptr, "null argument") TRY(orders, nullptr, "null argument") TRY(work, nullptr, "null argument")
  TRY(paths, nullptr, "null argument") TRY(status, nullptr, "null argument") TRY(arrive, nullptr, "null argument")
  TRY(key, nullptr, "null argument") TRY(best, nullptr, "null argument") TRY(serve_at, nullptr, "null argument")
  TRY(served, nullptr, "null argument") TRY(unserved, nullptr, "null argument")
  TRY(struct_size, 0, "struct_size") TRY(struct_size, (int32_t)sizeof(rmpc_timed_plan), "struct_size")
  TRY(struct_size, (int32_t)sizeof(rmpc_timed_tours) + 8, "struct_size")
  TRY(K, 0, "RMPC_TIMED_TOURS_MAX_STOPS") TRY(K, 65, "RMPC_TIMED_TOURS_MAX_STOPS") TRY(K, INT_MIN, "RMPC_TIMED_TOURS_MAX_STOPS")
  TRY(K, INT_MAX, "RMPC_TIMED_TOURS_MAX_STOPS")
  TRY(dwell, -1, "RMPC_TIMED_TOURS_MAX_DWELL") TRY(dwell, 65, "RMPC_TIMED_TOURS_MAX_DWELL")
  TRY(dwell, INT_MIN, "RMPC_TIMED_TOURS_MAX_DWELL") TRY(dwell, INT_MAX, "RMPC_TIMED_TOURS_MAX_DWELL")
  TRY(B, 0, "RMPC_TIMED_MAX_ROBOTS") TRY(B, 1025, "RMPC_TIMED_MAX_ROBOTS") TRY(B, INT_MIN, "RMPC_TIMED_MAX_ROBOTS")
  TRY(T, 0, "RMPC_TIMED_MAX_T") TRY(T, 1024, "RMPC_TIMED_MAX_T") TRY(T, INT_MAX, "RMPC_TIMED_MAX_T")
  TRY(sep2, 0, "RMPC_TIMED_MAX_SEP2") TRY(sep2, 4097, "RMPC_TIMED_MAX_SEP2")
  TRY(lag, 0, "lag must lie") TRY(lag, 5, "lag must lie") TRY(lag, INT_MIN, "lag must lie")
  TRY(G, 0, "RMPC_TIMED_MAX_ORDERS") TRY(G, 1025, "RMPC_TIMED_MAX_ORDERS") TRY(G, INT_MAX, "RMPC_TIMED_MAX_ORDERS")
  TRY(movement, 6, "") TRY(H, 0, "") TRY(W, 0, "") TRY(H, INT_MAX, "") TRY(Gf, 0, "") TRY(Gf, INT_MAX, "")
  TRY(work_bytes, full - 1, "the workspace holds") TRY(work_bytes, 0, "the workspace holds")
  TRY(work_bytes, INT64_MIN, "the workspace holds")
#undef TRY
  refused(rmpc_timed_tours_plan_device(nullptr, nullptr), "null argument", "p = nullptr");
  const int sizes[][4] = {{0, 5, 9, 2}, {7, 0, 9, 2}, {129, 128, 9, 1}, {7, 5, 0, 2}, {7, 5, 1024, 2}, {7, 5, 9, 0}, {7, 5, 9, 1025},
                          {INT_MAX, INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN, INT_MIN}};
  for (const auto &a : sizes) refused(rmpc_timed_tours_work_bytes(a[0], a[1], a[2], a[3]), "timed tours", "query");

  FollowArgs f;
  f.paths = f.idx_in = f.serve_at = (const int32_t *)buf;
  f.idx_out = (int32_t *)(buf + 8);
  f.leg = f.served = (int32_t *)buf;
  f.pos = f.goal = buf;
#define TRY(field, value, want)                    \
  {                                                \
    FollowArgs a = f;                              \
    a.field = value;                               \
    refused(follow(a), want, #field " = " #value); \
  }
  TRY(paths, nullptr, "null argument") TRY(idx_in, nullptr, "null argument") TRY(idx_out, nullptr, "null argument")
  TRY(pos, nullptr, "null argument") TRY(goal, nullptr, "null argument") TRY(serve_at, nullptr, "null argument")
  TRY(leg, nullptr, "null argument") TRY(served, nullptr, "null argument")
  TRY(idx_out, (int32_t *)buf, "d_idx_out must not be d_idx_in")
  TRY(B, 0, "RMPC_TIMED_MAX_ROBOTS") TRY(B, 1025, "RMPC_TIMED_MAX_ROBOTS") TRY(T, 0, "RMPC_TIMED_MAX_T")
  TRY(T, INT_MAX, "RMPC_TIMED_MAX_T") TRY(sep2, 0, "RMPC_TIMED_MAX_SEP2") TRY(lag, 0, "lag must lie") TRY(lag, 5, "lag must lie")
  TRY(K, 0, "RMPC_TIMED_TOURS_MAX_STOPS") TRY(K, 65, "RMPC_TIMED_TOURS_MAX_STOPS") TRY(K, INT_MIN, "RMPC_TIMED_TOURS_MAX_STOPS")
  TRY(stride, 1, "stride >= 2") TRY(stride, INT_MAX, "stride >= 2") TRY(W, 0, "W >= 1")
  TRY(stop_tol, -0.1, "stop_tol") TRY(stop_tol, NAN, "stop_tol") TRY(stop_tol, -INFINITY, "stop_tol")
#undef TRY
  std::printf(g_bad ? "FAILED: %d\n" : "timed tours refusals: all refused, no sanitizer report\n", g_bad);
  return g_bad ? 1 : 0;
}
