// Host check of the pass kernels' store after the recursion (csrc/rmpc_inst.hpp): store_after_recursion must leave in
// the workspace what inst_load -> inst_after_recursion -> inst_store leaves there, for every outcome of the recursion
// and every kernel variant, so that a rule added to inst_after_recursion cannot be forgotten in the store list.  A
// program of its own, compiled for x86 through tests/host/host_prelude.h; tests/test_after_recursion_host.py builds
// and runs it.  Test infrastructure only: nothing in the product includes or links this file.
#include "host_prelude.h"

#include <cstdio>
#include <cstring>

// (device-only in HIP's headers; inst_load / inst_store move the step lengths through them)
__attribute__((host)) static inline long long __double_as_longlong(double x) { long long r; std::memcpy(&r, &x, 8); return r; }
__attribute__((host)) static inline double __longlong_as_double(long long x) { double r; std::memcpy(&r, &x, 8); return r; }

#include "../../robot_mpcs_amd/csrc/rmpc_kernels.hip"   // (the device code)

namespace {
using namespace rmpc;

// The solver words of one instance, every word an array of its own length 1 inside one block that can be compared whole.
struct Words {
  double d[20];
  unsigned long long u[2];
  int i[20];
};
Ws bind(Words &m) {
  Ws W = {};
  W.N = 1; W.Bp = 1;
  int nd = 0, ni = 0;
  for (double **p : {&W.mu, &W.rho, &W.phi0, &W.Dd, &W.fcur, &W.thcur, &W.logcur, &W.res_stat, &W.res_eq, &W.res_ineq,
                     &W.res_comp, &W.obj, &W.mu_hold, &W.theta_mem, &W.theta_c})
    *p = &m.d[nd++];
  W.amin_p = &m.u[0]; W.amin_d = &m.u[1];
  for (int **p : {&W.status, &W.iters, &W.ls, &W.ls0, &W.lsst, &W.cur, &W.newstep, &W.redo, &W.force_gn, &W.gn_sticky,
                  &W.curv_fail, &W.usedc, &W.stall, &W.curv_skip, &W.curv_back, &W.small_steps, &W.theta_clean, &W.theta_retry})
    *p = &m.i[ni++];
  return W;
}
void fill(Words &m, const double theta_c, const int curv_back) {
  std::memset(&m, 0, sizeof m);
  for (int j = 0; j < 20; j++) { m.d[j] = 1000.5 + j; m.i[j] = 1000 + j; }
  m.u[0] = (unsigned long long)__double_as_longlong(0.75);
  m.u[1] = (unsigned long long)__double_as_longlong(0.625);
  const Ws W = bind(m);
  *W.theta_c = theta_c;
  *W.curv_back = curv_back;
}

template <class C>
int check(const char *name) {
  int bad = 0, n = 0;
  const double thetas[4] = {0.2, 0.3, 0.31, 1.0};   // around kCsMin
  const int backs[4] = {0, 1, 8, 16};               // up to kCurvBackMax
  for (int chol_ok = 0; chol_ok < 2; chol_ok++)
    for (int usec = 0; usec < 2; usec++)
      for (const double th : thetas)
        for (const int cb : backs) {
          Words a, r;
          fill(a, th, cb);
          fill(r, th, cb);
          const Ws Wa = bind(a), Wr = bind(r);
          store_after_recursion<C>(Wa, 0, chol_ok != 0, usec != 0, *Wa.theta_c, *Wa.curv_back);
          Inst s;
          inst_load(s, Wr, 0);
          inst_after_recursion(s, chol_ok != 0, usec != 0, C::BACKOFF, C::CSCALE);
          inst_store(s, Wr, 0);
          n++;
          if (std::memcmp(&a, &r, sizeof a) != 0) {
            bad++;
            std::printf("MISMATCH %s chol_ok=%d usec=%d theta_c=%g curv_back=%d\n", name, chol_ok, usec, th, cb);
            for (int j = 0; j < 20; j++) {
              if (a.d[j] != r.d[j]) std::printf("  double word %d: %g, rule %g\n", j, a.d[j], r.d[j]);
              if (a.i[j] != r.i[j]) std::printf("  int word %d: %d, rule %d\n", j, a.i[j], r.i[j]);
            }
            for (int j = 0; j < 2; j++)
              if (a.u[j] != r.u[j]) std::printf("  step length %d: %llx, rule %llx\n", j, a.u[j], r.u[j]);
          }
        }
  std::printf("%s BACKOFF=%d CSCALE=%d: %d cases, %d mismatches\n", name, (int)C::BACKOFF, (int)C::CSCALE, n, bad);
  return bad;
}
}  // namespace

int main() {
  int bad = 0;
  // the rows of RMPC_VARIANTS (csrc/rmpc_variants.hip): between them every combination of BACKOFF / CSCALE in use
#define CHECK(robot, n, ns) bad += check<Cfg<robot, n, ns>>("Cfg<" #robot ", " #n ", " #ns ">");
  CHECK(RMPC_ROBOT_CHAIN, 3, 0) CHECK(RMPC_ROBOT_CHAIN, 3, 1) CHECK(RMPC_ROBOT_CHAIN, 7, 0) CHECK(RMPC_ROBOT_CHAIN, 7, 1)
  CHECK(RMPC_ROBOT_DIFFDRIVE, 3, 0) CHECK(RMPC_ROBOT_DIFFDRIVE, 3, 1) CHECK(RMPC_ROBOT_CHAIN, 2, 0) CHECK(RMPC_ROBOT_CHAIN, 4, 0)
  CHECK(RMPC_ROBOT_CHAIN, 5, 0) CHECK(RMPC_ROBOT_CHAIN, 6, 0) CHECK(RMPC_ROBOT_CHAIN, 8, 0)
#undef CHECK
  std::printf(bad ? "FAILED\n" : "OK\n");
  return bad ? 1 : 0;
}
