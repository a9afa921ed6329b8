// The host side of the large-map fields under AddressSanitizer + UBSan, as a program of its own: the argument checks of
// rmpc_grid_fields_large_device and rmpc_grid_fields_seeded_large_device (rmpc_world.hip, include/rmpc_grid_large.h) are
// plain C++ that runs before any HIP call.  Every call below is refused (-1 with the entry's message); the pointers are
// never read.
//   bash tests/host/run_refusals.sh grid_large
#include "../../robot_mpcs_amd/csrc/rmpc_world.hip"

#include <cstdio>
#include <limits>

static int g_bad = 0;
static void refused(int rc, const char *want, const char *what) {
  if (rc != -1 || g_err != want) {
    std::printf("NOT REFUSED %s: rc %d, message '%s', expected '%s'\n", what, rc, g_err.c_str(), want);
    g_bad++;
  }
}

struct Args {
  int H = 300, W = 300;
  const double *grid;
  int G = 1;
  const void *src;
  int movement = 8;
  double occ = 0.8, f = 3.0;
  double *fields;
  int32_t *status;
};

static void both(const Args &a, const char *want, const char *what) {
  refused(rmpc_grid_fields_large_device(a.H, a.W, a.grid, a.G, (const int32_t *)a.src, a.movement, a.occ, a.f, a.fields,
                                        a.status, nullptr, nullptr), want, what);
  refused(rmpc_grid_fields_seeded_large_device(a.H, a.W, a.grid, a.G, (const double *)a.src, a.movement, a.occ, a.f,
                                               a.fields, a.status, nullptr, nullptr), want, what);
}

int main() {
  static double buf[64];
  Args ok;
  ok.grid = buf; ok.src = buf; ok.fields = buf; ok.status = (int32_t *)buf;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
#define TRY(field, value, want)       \
  {                                   \
    Args t = ok;                      \
    t.field = value;                  \
    both(t, want, #field " = " #value); \
  }
#define TRY2(f1, v1, f2, v2, want)                     \
  {                                                    \
    Args t = ok;                                       \
    t.f1 = v1;                                         \
    t.f2 = v2;                                         \
    both(t, want, #f1 " = " #v1 ", " #f2 " = " #v2);   \
  }
  TRY(grid, nullptr, "null argument") TRY(src, nullptr, "null argument") TRY(fields, nullptr, "null argument")
  TRY(status, nullptr, "null argument")
  const char *hw = "grid fields large: need H, W >= 1";
  TRY(H, 0, hw) TRY(W, 0, hw) TRY(H, -1, hw) TRY(H, INT_MIN, hw) TRY(W, INT_MIN, hw) TRY2(H, INT_MIN, W, INT_MIN, hw)
  const char *mv = "grid fields large: movement must be 4 or 8";
  TRY(movement, 0, mv) TRY(movement, 5, mv) TRY(movement, INT_MAX, mv) TRY(movement, INT_MIN, mv)
  TRY2(H, 8193, W, 1, "grid fields large: 8193x1 map has a side above RMPC_GRID_LARGE_MAX_SIDE = 8192")
  TRY(W, INT_MAX, "grid fields large: 300x2147483647 map has a side above RMPC_GRID_LARGE_MAX_SIDE = 8192")
  TRY2(H, INT_MAX, W, INT_MAX, "grid fields large: 2147483647x2147483647 map has a side above RMPC_GRID_LARGE_MAX_SIDE = 8192")
  TRY2(H, 2049, W, 2048, "grid fields large: 2049x2048 map exceeds RMPC_GRID_LARGE_MAX_CELLS = 4194304 cells")
  TRY2(H, 8192, W, 8192, "grid fields large: 8192x8192 map exceeds RMPC_GRID_LARGE_MAX_CELLS = 4194304 cells")
  const char *ghw = "grid fields large: need 1 <= G and G*H*W <= INT_MAX";
  TRY(G, 0, ghw) TRY(G, -1, ghw) TRY(G, INT_MIN, ghw) TRY(G, INT_MAX, ghw)
  {
    Args t = ok;
    t.H = t.W = 2048; t.G = 512;      // 2^31 cells
    both(t, ghw, "G H W = 2^31");
  }
  const char *cost = "grid fields large: cost_factor must be finite and >= 0";
  TRY(f, -1.0, cost) TRY(f, nan, cost) TRY(f, inf, cost) TRY(f, -inf, cost)
#undef TRY
#undef TRY2
  std::printf(g_bad ? "FAILED: %d\n" : "grid large refusals: all refused, no sanitizer report\n", g_bad);
  return g_bad ? 1 : 0;
}
