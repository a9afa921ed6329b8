// The host side of the timed routes with repaired orders under AddressSanitizer + UBSan, as a program of its own: the
// argument checks of rmpc_timed_plan_repair_device and its size query (rmpc_world.hip) are plain C++ that runs before
// any HIP call.  Every call below is refused (-1 with the entry's message); the pointers are never read.
//   bash tests/host/run_refusals.sh timed_repair
#include "../../robot_mpcs_amd/csrc/rmpc_world.hip"

#include <cstdio>

static int g_bad = 0;
static void refused(long long rc, const char *want, const char *what) {
  if (rc != -1 || g_err.find(want) == std::string::npos) {
    std::printf("NOT REFUSED %s: rc %lld, message '%s'\n", what, rc, g_err.c_str());
    g_bad++;
  }
}

int main() {
  static double buf[64];
  rmpc_timed_repair t = {};
  t.struct_size = (int32_t)sizeof(rmpc_timed_repair);
  t.H = 7; t.W = 5; t.movement = 4;
  t.grid = t.fields = buf;
  t.occ_threshold = 0.8;
  t.B = 3; t.Gf = 2;
  t.start_cell = t.goal_index = t.goal_cells = t.orders = (const int32_t *)buf;
  t.T = 9; t.sep2 = 2; t.lag = 1; t.G = 2;
  t.work = buf; t.work_bytes = 1 << 20;
  t.paths = t.status = t.arrive = t.best = t.order_out = t.rounds_run = t.round_best = (int32_t *)buf;
  t.key = (int64_t *)buf;
  t.rounds = 2;
  const int64_t full = rmpc_timed_plan_repair_work_bytes(7, 5, 9, 2, 3);
  if (full != rmpc_timed_plan_work_bytes(7, 5, 9, 2) + 2 * 8 * ((3 * 10 + 4 * 3 + 1) / 2) ||
      rmpc_timed_plan_repair_work_bytes(128, 128, 1023, 1024, 1024) !=
          rmpc_timed_plan_work_bytes(128, 128, 1023, 1024) + 1024LL * 8 * ((1024LL * 1024 + 4 * 1024 + 1) / 2)) {
    std::printf("sizes %lld\n", (long long)full);
    g_bad++;
  }
#define TRY(field, value, want)                                                     \
  {                                                                                 \
    rmpc_timed_repair a = t;                                                        \
    a.field = value;                                                                \
    refused(rmpc_timed_plan_repair_device(&a, nullptr), want, #field " = " #value); \
  }
  TRY(grid, nullptr, "null argument") TRY(start_cell, nullptr, "null argument") TRY(goal_index, nullptr, "null argument")
  TRY(fields, nullptr, "null argument") TRY(goal_cells, nullptr, "null argument") TRY(orders, nullptr, "null argument")
  TRY(work, nullptr, "null argument") TRY(paths, nullptr, "null argument") TRY(status, nullptr, "null argument")
  TRY(arrive, nullptr, "null argument") TRY(key, nullptr, "null argument") TRY(best, nullptr, "null argument")
  TRY(order_out, nullptr, "null argument") TRY(rounds_run, nullptr, "null argument") TRY(round_best, nullptr, "null argument")
  TRY(struct_size, 0, "rmpc_timed_repair.struct_size") TRY(struct_size, (int32_t)sizeof(rmpc_timed_repair) - 8, "rmpc_timed_repair.struct_size")
  TRY(struct_size, (int32_t)sizeof(rmpc_timed_plan), "rmpc_timed_repair.struct_size")
  TRY(rounds, -1, "RMPC_TIMED_MAX_ROUNDS") TRY(rounds, 17, "RMPC_TIMED_MAX_ROUNDS") TRY(rounds, INT_MAX, "RMPC_TIMED_MAX_ROUNDS")
  TRY(rounds, INT_MIN, "RMPC_TIMED_MAX_ROUNDS")
  TRY(B, 0, "RMPC_TIMED_MAX_ROBOTS") TRY(B, 1025, "RMPC_TIMED_MAX_ROBOTS") TRY(B, INT_MIN, "RMPC_TIMED_MAX_ROBOTS")
  TRY(T, 0, "RMPC_TIMED_MAX_T") TRY(T, 1024, "RMPC_TIMED_MAX_T") TRY(T, INT_MAX, "RMPC_TIMED_MAX_T")
  TRY(sep2, 0, "RMPC_TIMED_MAX_SEP2") TRY(sep2, 4097, "RMPC_TIMED_MAX_SEP2")
  TRY(lag, 0, "lag must lie") TRY(lag, 5, "lag must lie") TRY(lag, INT_MIN, "lag must lie")
  TRY(G, 0, "RMPC_TIMED_MAX_ORDERS") TRY(G, 1025, "RMPC_TIMED_MAX_ORDERS") TRY(G, INT_MAX, "RMPC_TIMED_MAX_ORDERS")
  TRY(movement, 6, "") TRY(H, 0, "") TRY(W, 0, "") TRY(H, INT_MAX, "") TRY(Gf, 0, "") TRY(Gf, INT_MAX, "")
  TRY(work_bytes, full - 1, "the workspace holds") TRY(work_bytes, 0, "the workspace holds")
  TRY(work_bytes, INT64_MIN, "the workspace holds")
  TRY(work_bytes, rmpc_timed_plan_work_bytes(7, 5, 9, 2), "rmpc_timed_plan_repair_work_bytes")    // the plan's size is too small
#undef TRY
  refused(rmpc_timed_plan_repair_device(nullptr, nullptr), "null argument", "p = nullptr");
  const int sizes[][5] = {{0, 5, 9, 2, 3}, {7, 0, 9, 2, 3}, {129, 128, 9, 1, 3}, {7, 5, 0, 2, 3}, {7, 5, 1024, 2, 3},
                          {7, 5, 9, 0, 3}, {7, 5, 9, 1025, 3}, {7, 5, 9, 2, 0}, {7, 5, 9, 2, 1025}, {7, 5, 9, 2, INT_MIN},
                          {INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN, INT_MIN, INT_MIN}};
  for (const auto &a : sizes) refused(rmpc_timed_plan_repair_work_bytes(a[0], a[1], a[2], a[3], a[4]), "timed repair", "work query");
  std::printf(g_bad ? "FAILED: %d\n" : "timed repair refusals: all refused, no sanitizer report\n", g_bad);
  return g_bad ? 1 : 0;
}
