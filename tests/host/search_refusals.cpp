// The host side of wide-window localisation under AddressSanitizer + UBSan, as a program of its own: the argument checks
// of rmpc_grid_min_pyramid_device and rmpc_scan_search_device and the work-size query (rmpc_world.hip) are plain C++ that
// runs before any HIP call.  Every call below is refused (-1 with the entry's message); the pointers are never read.
//   bash tests/host/run_refusals.sh search
#include "../../robot_mpcs_amd/csrc/rmpc_world.hip"

#include <cstdio>
#include <cstring>

static int g_bad = 0;
static void refused(long long rc, const char *want, const char *what) {
  if (rc != -1 || g_err.find(want) == std::string::npos) {
    std::printf("NOT REFUSED %s: rc %lld, message '%s'\n", what, rc, g_err.c_str());
    g_bad++;
  }
}

int main() {
  static double buf[64];
  void *const P = buf;
  rmpc_scan_search s;
  std::memset(&s, 0, sizeof s);
  s.struct_size = (int32_t)sizeof s;
  s.rays = 4; s.range = 10.0; s.pose_stride = 8; s.min_hits = 1;
  s.H = 2; s.W = 2; s.sub = 2; s.cap = 16; s.cell = 0.5;
  s.nxy = 3; s.nth = 1; s.step_xy = 0.03; s.step_th = 0.01; s.levels = 2; s.top_log2 = 1;
  s.pose = s.points = s.ranges = s.rot = (const double *)P;
  s.d2 = s.pyr = (const int32_t *)P;
  s.pose_out = (double *)P; s.best = s.score = (int32_t *)P;
  s.work = P;
  const int64_t full = rmpc_scan_search_work_bytes(1, 3, 1, 1);
  if (full != 4 * 3 * 4 * 4) { std::printf("work bytes %lld\n", (long long)full); g_bad++; }
  s.work_bytes = full;
#define TRY(field, value, want)                                  \
  {                                                              \
    rmpc_scan_search t = s;                                      \
    t.field = value;                                             \
    refused(rmpc_scan_search_device(1, &t, nullptr), want, #field " = " #value); \
  }
  TRY(struct_size, 8, "struct_size mismatch")
  TRY(nxy, -1, "[0, 127]") TRY(nxy, 128, "[0, 127]") TRY(nth, -1, "[0, 127]") TRY(nth, 128, "[0, 127]")
  TRY(top_log2, -1, "top_log2") TRY(top_log2, 8, "top_log2") TRY(top_log2, INT_MAX, "top_log2")
  TRY(levels, 0, "levels") TRY(levels, 13, "levels") TRY(levels, INT_MIN, "levels")
  TRY(pyr, nullptr, "null argument") TRY(work, nullptr, "null argument") TRY(d2, nullptr, "null argument")
  TRY(work_bytes, full - 1, "work_bytes") TRY(work_bytes, -1, "work_bytes") TRY(work_bytes, INT64_MIN, "work_bytes")
  TRY(rays, 0, "RMPC_MATCH_MAX_RAYS") TRY(min_hits, 0, "min_hits") TRY(step_xy, 0.0, "a step of 0")
  TRY(cap, 65536, "cap must lie") TRY(H, 0, "need H, W") TRY(H, 1 << 20, "RMPC_GRID_MAX_CELLS") TRY(cell, 0.0, "cell must be positive")
#undef TRY
  refused(rmpc_scan_search_device(0, &s, nullptr), "need B >= 1", "B = 0");
  refused(rmpc_scan_search_device(1, nullptr, nullptr), "null argument", "NULL struct");
  {                                                               // B ntop beyond INT_MAX, and its workspace beyond 2^32
    rmpc_scan_search t = s;
    t.nxy = t.nth = 127; t.top_log2 = 0; t.rays = 1; t.pose_stride = 3;
    t.work_bytes = INT64_MAX;
    refused(rmpc_scan_search_device(200, &t, nullptr), "INT_MAX", "B ntop");
  }
  const int args[][4] = {{0, 3, 1, 1}, {-1, 3, 1, 1}, {1, 128, 1, 1}, {1, -1, 1, 1}, {1, 3, 128, 1}, {1, 3, -1, 1},
                         {1, 3, 1, 8}, {1, 3, 1, -1}, {1, INT_MAX, INT_MAX, 31}, {INT_MIN, INT_MIN, INT_MIN, INT_MIN}};
  for (const auto &a : args) refused(rmpc_scan_search_work_bytes(a[0], a[1], a[2], a[3]), "scan search work bytes", "query");
  if (rmpc_scan_search_work_bytes(INT_MAX, 127, 127, 0) != (int64_t)INT_MAX * 255 * 255 * 255 * 4) {
    std::printf("largest work size wrong\n");
    g_bad++;
  }
  refused(rmpc_grid_min_pyramid_device(2, 2, 2, nullptr, 2, (int32_t *)P, nullptr), "null argument", "pyramid d2");
  refused(rmpc_grid_min_pyramid_device(2, 2, 2, (const int32_t *)P, 2, nullptr, nullptr), "null argument", "pyramid pyr");
  refused(rmpc_grid_min_pyramid_device(0, 2, 2, (const int32_t *)P, 2, (int32_t *)P, nullptr), "need H, W", "pyramid H");
  refused(rmpc_grid_min_pyramid_device(129, 128, 2, (const int32_t *)P, 2, (int32_t *)P, nullptr), "RMPC_GRID_MAX_CELLS", "pyramid cells");
  refused(rmpc_grid_min_pyramid_device(2, 2, 9, (const int32_t *)P, 2, (int32_t *)P, nullptr), "sub must lie", "pyramid sub");
  refused(rmpc_grid_min_pyramid_device(2, 2, 2, (const int32_t *)P, 0, (int32_t *)P, nullptr), "levels", "pyramid levels 0");
  refused(rmpc_grid_min_pyramid_device(2, 2, 2, (const int32_t *)P, 13, (int32_t *)P, nullptr), "levels", "pyramid levels 13");
  std::printf(g_bad ? "FAILED: %d\n" : "search refusals: all refused, no sanitizer report\n", g_bad);
  return g_bad ? 1 : 0;
}
