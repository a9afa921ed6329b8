// The host side of the tours under AddressSanitizer + UBSan, as a program of its own: the argument checks of
// rmpc_tours_device and rmpc_follow_tour_device and the work-size query (rmpc_world.hip) are plain C++ that runs before
// any HIP call.  Every call below is refused (-1 with the entry's message); the pointers are never read.
//   bash tests/host/run_refusals.sh tours
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

struct ToursArgs {
  int G = 1, B = 4, T = 6, K = 2;
  const double *start, *task;
  int mode = 1;
  double scale = 1024.0;
  int max_rounds = 5;
  int32_t *tours, *len;
  int64_t *cost;
  void *work;
  int64_t bytes = 1 << 20;
};
static long long tours(const ToursArgs &a) {
  return rmpc_tours_device(a.G, a.B, a.T, a.K, a.start, a.task, a.mode, a.scale, a.max_rounds, a.tours, a.len, a.cost,
                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, a.work, a.bytes, nullptr);
}

struct FollowArgs {
  int B = 2, max_len = 8, stride = 3, W = 41, K = 2, now = 0;
  const int32_t *path, *len, *stop_at;
  int32_t *idx, *leg, *served;
  const double *pos;
  double *goal;
  double stop_tol = 0.2;
};
static long long follow(const FollowArgs &a) {
  return rmpc_follow_tour_device(a.B, a.path, a.len, a.max_len, a.idx, a.pos, a.stride, a.W, 0.0, 0.0, 0.5, 1.3, a.goal,
                                 a.K, a.stop_at, a.leg, a.served, a.now, a.stop_tol, nullptr);
}

int main() {
  static double buf[64];
  ToursArgs t;
  t.start = t.task = buf;
  t.tours = t.len = (int32_t *)buf;
  t.cost = (int64_t *)buf;
  t.work = buf;
  const int64_t full = rmpc_tours_work_bytes(1, 4, 6);
  if (full != 4 * (72 + 72)) { std::printf("work bytes %lld\n", (long long)full); g_bad++; }
#define TRY(field, value, want)                   \
  {                                               \
    ToursArgs a = t;                              \
    a.field = value;                              \
    refused(tours(a), want, #field " = " #value); \
  }
  TRY(start, nullptr, "null argument") TRY(task, nullptr, "null argument") TRY(tours, nullptr, "null argument")
  TRY(len, nullptr, "null argument") TRY(cost, nullptr, "null argument") TRY(work, nullptr, "null argument")
  TRY(B, 0, "RMPC_TOURS_MAX_ROBOTS") TRY(B, 1025, "RMPC_TOURS_MAX_ROBOTS") TRY(B, INT_MIN, "RMPC_TOURS_MAX_ROBOTS")
  TRY(T, 0, "RMPC_TOURS_MAX_TASKS") TRY(T, 1025, "RMPC_TOURS_MAX_TASKS") TRY(T, INT_MAX, "RMPC_TOURS_MAX_TASKS")
  TRY(G, 0, "1 <= G") TRY(G, -1, "1 <= G") TRY(G, INT_MIN, "1 <= G") TRY(G, INT_MAX, "1 <= G")
  TRY(K, 0, "1 <= K <= T") TRY(K, 7, "1 <= K <= T") TRY(K, INT_MIN, "1 <= K <= T") TRY(K, INT_MAX, "1 <= K <= T")
  TRY(mode, 2, "mode must be") TRY(mode, -1, "mode must be") TRY(mode, INT_MAX, "mode must be")
  TRY(scale, 0.0, "scale must be") TRY(scale, -1.0, "scale must be") TRY(scale, NAN, "scale must be")
  TRY(scale, INFINITY, "scale must be")
  TRY(max_rounds, -1, "max_rounds") TRY(max_rounds, INT_MIN, "max_rounds")
  TRY(bytes, full - 1, "the workspace holds") TRY(bytes, 0, "the workspace holds") TRY(bytes, -1, "the workspace holds")
  TRY(bytes, INT64_MIN, "the workspace holds")
#undef TRY
  {                                                               // G T T beyond INT_MAX with every size within its limit
    ToursArgs a = t;
    a.G = 2048; a.B = 1; a.T = 1024; a.K = 1; a.bytes = INT64_MAX;
    refused(tours(a), "G*T*T <= INT_MAX", "G T T");
    a.G = 2047;                                                   // the largest G at T = 1024: the query answers
    if (rmpc_tours_work_bytes(a.G, a.B, a.T) != 4ll * 2047 * (3 * 1024 + 2 * 1024 * 1024)) { std::printf("largest work size wrong\n"); g_bad++; }
  }
  const int args[][3] = {{0, 4, 6}, {-1, 4, 6}, {1, 0, 6}, {1, 1025, 6}, {1, 4, 0}, {1, 4, 1025}, {2048, 1, 1024},
                         {INT_MAX, 1024, 1}, {INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN}};
  for (const auto &a : args) refused(rmpc_tours_work_bytes(a[0], a[1], a[2]), "tours work bytes", "query");
  if (rmpc_tours_work_bytes(INT_MAX, 1, 1) != 20ll * INT_MAX) { std::printf("G = INT_MAX work size wrong\n"); g_bad++; }

  FollowArgs f;
  f.path = f.len = f.stop_at = (const int32_t *)buf;
  f.idx = f.leg = f.served = (int32_t *)buf;
  f.pos = f.goal = buf;
#define TRY(field, value, want)                    \
  {                                                \
    FollowArgs a = f;                              \
    a.field = value;                               \
    refused(follow(a), want, #field " = " #value); \
  }
  TRY(path, nullptr, "null argument") TRY(len, nullptr, "null argument") TRY(idx, nullptr, "null argument")
  TRY(pos, nullptr, "null argument") TRY(goal, nullptr, "null argument") TRY(stop_at, nullptr, "null argument")
  TRY(leg, nullptr, "null argument") TRY(served, nullptr, "null argument")
  TRY(B, 0, "B, max_len >= 1") TRY(B, INT_MIN, "B, max_len >= 1") TRY(max_len, 0, "B, max_len >= 1")
  TRY(max_len, INT_MAX, "B*max_len <= INT_MAX")
  TRY(K, 0, "K >= 1") TRY(K, INT_MIN, "K >= 1") TRY(K, INT_MAX, "B*K <= INT_MAX")
  TRY(stride, 1, "stride >= 2") TRY(stride, INT_MAX, "stride >= 2") TRY(W, 0, "W >= 1")
  TRY(stop_tol, -0.1, "stop_tol") TRY(stop_tol, NAN, "stop_tol") TRY(stop_tol, -INFINITY, "stop_tol")
#undef TRY
  std::printf(g_bad ? "FAILED: %d\n" : "tours refusals: all refused, no sanitizer report\n", g_bad);
  return g_bad ? 1 : 0;
}
