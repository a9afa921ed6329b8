// The host side of the lifelong timed tours under AddressSanitizer + UBSan, as a program of its own: the argument checks
// of rmpc_timed_reserve_device and rmpc_timed_tours_replan_device and the two size queries (rmpc_world.hip) are plain
// C++ that runs before any HIP call.  Every call below is refused (-1 with the entry's message); the pointers are never
// read.
//   bash tests/host/run_refusals.sh timed_replan
#include "../../robot_mpcs_amd/csrc/rmpc_world.hip"

#include <cstdio>

static int g_bad = 0;
static void refused(long long rc, const char *want, const char *what) {
  if (rc != -1 || g_err.find(want) == std::string::npos) {
    std::printf("NOT REFUSED %s: rc %lld, message '%s'\n", what, rc, g_err.c_str());
    g_bad++;
  }
}

struct ReserveArgs {
  int H = 7, W = 5, T = 9, P = 3, sep2 = 2, lag = 1, clear = 1;
  const int32_t *cells, *use = nullptr;
  uint64_t *res;
};
static long long reserve(const ReserveArgs &a) {
  return rmpc_timed_reserve_device(a.H, a.W, a.T, a.P, a.cells, a.use, a.sep2, a.lag, a.clear, a.res, nullptr);
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
  t.work = nullptr; t.work_bytes = 0;                      // (not read)
  t.paths = t.status = t.arrive = t.best = t.serve_at = t.served = t.unserved = (int32_t *)buf;
  t.key = (int64_t *)buf;
  rmpc_timed_replan x = {};
  x.struct_size = (int32_t)sizeof(rmpc_timed_replan);
  x.work = buf; x.work_bytes = 1 << 20;
  const int64_t full = rmpc_timed_replan_work_bytes(7, 5, 9, 2);
  if (full != rmpc_timed_tours_work_bytes(7, 5, 9, 2) + 8 * ((1024 + 4 + 3 * 35 + 1) / 2) ||
      rmpc_timed_reserve_words(7, 5, 9) != 70 || rmpc_timed_reserve_words(4, 130, 40) != 41 * 4 * 3) {
    std::printf("sizes %lld\n", (long long)full);
    g_bad++;
  }
#define TRY(field, value, want)                                                            \
  {                                                                                        \
    rmpc_timed_tours a = t;                                                                \
    a.field = value;                                                                       \
    refused(rmpc_timed_tours_replan_device(&a, &x, nullptr), want, #field " = " #value);   \
  }
  TRY(grid, nullptr, "null argument") TRY(start_cell, nullptr, "null argument") TRY(stops, nullptr, "null argument")
  TRY(len, nullptr, "null argument") TRY(park_index, nullptr, "null argument") TRY(fields, nullptr, "null argument")
  TRY(goal_cells, nullptr, "null argument") TRY(orders, nullptr, "null argument")
  TRY(paths, nullptr, "null argument") TRY(status, nullptr, "null argument") TRY(arrive, nullptr, "null argument")
  TRY(key, nullptr, "null argument") TRY(best, nullptr, "null argument") TRY(serve_at, nullptr, "null argument")
  TRY(served, nullptr, "null argument") TRY(unserved, nullptr, "null argument")
  TRY(struct_size, 0, "rmpc_timed_tours.struct_size") TRY(struct_size, (int32_t)sizeof(rmpc_timed_tours) + 8, "rmpc_timed_tours.struct_size")
  TRY(K, 0, "RMPC_TIMED_TOURS_MAX_STOPS") TRY(K, 65, "RMPC_TIMED_TOURS_MAX_STOPS") TRY(K, INT_MIN, "RMPC_TIMED_TOURS_MAX_STOPS")
  TRY(dwell, -1, "RMPC_TIMED_TOURS_MAX_DWELL") TRY(dwell, 65, "RMPC_TIMED_TOURS_MAX_DWELL") TRY(dwell, INT_MAX, "RMPC_TIMED_TOURS_MAX_DWELL")
  TRY(B, 0, "RMPC_TIMED_MAX_ROBOTS") TRY(B, 1025, "RMPC_TIMED_MAX_ROBOTS") TRY(B, INT_MIN, "RMPC_TIMED_MAX_ROBOTS")
  TRY(T, 0, "RMPC_TIMED_MAX_T") TRY(T, 1024, "RMPC_TIMED_MAX_T") TRY(T, INT_MAX, "RMPC_TIMED_MAX_T")
  TRY(sep2, 0, "RMPC_TIMED_MAX_SEP2") TRY(sep2, 4097, "RMPC_TIMED_MAX_SEP2")
  TRY(lag, 0, "lag must lie") TRY(lag, 5, "lag must lie") TRY(lag, INT_MIN, "lag must lie")
  TRY(G, 0, "RMPC_TIMED_MAX_ORDERS") TRY(G, 1025, "RMPC_TIMED_MAX_ORDERS") TRY(G, INT_MAX, "RMPC_TIMED_MAX_ORDERS")
  TRY(movement, 6, "") TRY(H, 0, "") TRY(W, 0, "") TRY(H, INT_MAX, "") TRY(Gf, 0, "") TRY(Gf, INT_MAX, "")
#undef TRY
#define TRY(field, value, want)                                                            \
  {                                                                                        \
    rmpc_timed_replan a = x;                                                               \
    a.field = value;                                                                       \
    refused(rmpc_timed_tours_replan_device(&t, &a, nullptr), want, #field " = " #value);   \
  }
  TRY(struct_size, 0, "rmpc_timed_replan.struct_size") TRY(struct_size, (int32_t)sizeof(rmpc_timed_replan) - 8, "rmpc_timed_replan.struct_size")
  TRY(struct_size, (int32_t)sizeof(rmpc_timed_tours), "rmpc_timed_replan.struct_size")
  TRY(work, nullptr, "null argument")
  TRY(work_bytes, full - 1, "the workspace holds") TRY(work_bytes, 0, "the workspace holds")
  TRY(work_bytes, INT64_MIN, "the workspace holds")
  TRY(work_bytes, rmpc_timed_tours_work_bytes(7, 5, 9, 2), "rmpc_timed_replan_work_bytes")       // the tours' size is too small
#undef TRY
  refused(rmpc_timed_tours_replan_device(nullptr, &x, nullptr), "null argument", "p = nullptr");
  refused(rmpc_timed_tours_replan_device(&t, nullptr, nullptr), "null argument", "x = nullptr");
  const int sizes[][4] = {{0, 5, 9, 2}, {7, 0, 9, 2}, {129, 128, 9, 1}, {7, 5, 0, 2}, {7, 5, 1024, 2}, {7, 5, 9, 0}, {7, 5, 9, 1025},
                          {INT_MAX, INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN, INT_MIN}};
  for (const auto &a : sizes) refused(rmpc_timed_replan_work_bytes(a[0], a[1], a[2], a[3]), "timed replan", "work query");
  const int words[][3] = {{0, 5, 9}, {7, 0, 9}, {129, 128, 9}, {7, 5, 0}, {7, 5, 1024}, {INT_MAX, INT_MAX, INT_MAX},
                          {INT_MIN, INT_MIN, INT_MIN}};
  for (const auto &a : words) refused(rmpc_timed_reserve_words(a[0], a[1], a[2]), "timed reserve", "words query");

  ReserveArgs r;
  r.cells = (const int32_t *)buf;
  r.res = (uint64_t *)buf;
#define TRY(field, value, want)                     \
  {                                                 \
    ReserveArgs a = r;                              \
    a.field = value;                                \
    refused(reserve(a), want, #field " = " #value); \
  }
  TRY(cells, nullptr, "null argument") TRY(res, nullptr, "null argument")
  TRY(P, 0, "RMPC_TIMED_RESERVE_MAX_PATHS") TRY(P, 4097, "RMPC_TIMED_RESERVE_MAX_PATHS") TRY(P, INT_MIN, "RMPC_TIMED_RESERVE_MAX_PATHS")
  TRY(T, 0, "RMPC_TIMED_MAX_T") TRY(T, 1024, "RMPC_TIMED_MAX_T") TRY(T, INT_MAX, "RMPC_TIMED_MAX_T")
  TRY(sep2, 0, "RMPC_TIMED_MAX_SEP2") TRY(sep2, 4097, "RMPC_TIMED_MAX_SEP2") TRY(sep2, INT_MIN, "RMPC_TIMED_MAX_SEP2")
  TRY(lag, 0, "lag must lie") TRY(lag, 5, "lag must lie")
  TRY(H, 0, "") TRY(W, 0, "") TRY(H, INT_MAX, "") TRY(W, INT_MIN, "")
#undef TRY
  std::printf(g_bad ? "FAILED: %d\n" : "timed replan refusals: all refused, no sanitizer report\n", g_bad);
  return g_bad ? 1 : 0;
}
