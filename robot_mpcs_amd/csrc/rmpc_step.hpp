// rmpc_step.hpp -- the step lengths of a stage: step_body (fraction-to-the-boundary minima, merit slope partial), what
// it addresses (StepIO) and the pass kernel k_step.  Part of rmpc_kernels.hip (included there, inside namespace rmpc);
// needs rmpc_sweep.hpp (StepRow).

// ===========================================================================
// k_step: slack / multiplier steps and step-length partials, stage parallel
// ===========================================================================
// What one lane of the step kernel addresses (same convention as SweepIO).
template <class RP = gdouble>   // RP: where the step lives
struct StepIO {
  const gdouble *zc, *tc, *lc, *grow, *Jq, *gfa;
  const RP *dz;
  size_t SS;
  unsigned loff;
  size_t SSd;       // addressing of dz (see SweepIO)
  unsigned loffd;
};

// ap, ad: fraction-to-the-boundary step lengths of this stage (1 when no row binds); gphi: its merit slope partial
template <class C, class RP = gdouble, class V = RtView>
__device__ __forceinline__ void step_body(const V &v, const StepIO<RP> &io, const int k, const double mu,
                                          double &ap_out, double &ad_out, double &gphi_out) {
  constexpr int NQ = C::NQ, NX = C::NX, NS = C::NS, NV = C::NV;
  const unsigned loff = io.loff;
  const size_t SS = io.SS;
  const gdouble *__restrict__ zc = io.zc;
  const gdouble *__restrict__ tc = io.tc;
  const gdouble *__restrict__ lc = io.lc;
  const gdouble *__restrict__ grow = io.grow;
  const gdouble *__restrict__ Jq = io.Jq;
  double dz[NV], z[NV], gfv[NV];
#pragma unroll
  for (int j = 0; j < NV; j++) {
    dz[j] = io.dz[(size_t)j * io.SSd + io.loffd];
    z[j] = zc[IDXL(j)];
    gfv[j] = io.gfa[IDXL(j)];
  }
  StepRow<C> sr;   // (the row arithmetic: shared with the merged form in sweep_body)
  sr.slope(gfv, dz);
  // Every request of the phase leaves before the first row is evaluated (one wavefront per SIMD hides no latency by
  // itself; left where the arithmetic is, the compiler waits for each small group of loads in turn: a dozen round
  // trips to L2 per call instead of one).  The rows are then evaluated in the old order (the merit slope is a sum).
  struct FkIn { double g, tv, lv, jq[NQ]; };
  auto fk_load = [&](const int r, FkIn &f) __attribute__((always_inline)) {
    const int i = v.fk_row(r), fi = v.fk_idx(r);
    f.g = grow[IDXL(i)]; f.tv = tc[IDXL(i)]; f.lv = lc[IDXL(i)];
#pragma unroll
    for (int a = 0; a < NQ; a++) f.jq[a] = Jq[IDXL(fi * NQ + a)];
  };
  auto fk_row_body = [&](const int r, const FkIn &f) __attribute__((always_inline)) {
    (void)r;
    sr.template fk_row<V>(mu, dz, f.g, f.tv, f.lv, f.jq);
  };
  constexpr int NFKC = []() { if constexpr (V::SPEC) return V::nfkrows() > 0 ? V::nfkrows() : 1; else return 1; }();
  FkIn fkin[NFKC];
  if constexpr (V::SPEC) {
    for_range<0, V::nfkrows()>([&](auto rc) __attribute__((always_inline)) { fk_load(decltype(rc)::value, fkin[decltype(rc)::value]); });
  }
  // single-variable rows, by variable (unconditional clamped requests, see sweep_body), in chunks of VCH variables whose
  // requests leave together: all of them for the small models, one variable at a time for the arms (12 requests per
  // variable: more in flight cost the arm's kernel registers it does not have -- k_step 30 -> 33 us with six)
  constexpr int VCH = NV <= 12 ? NV : 1;
  double tvv[VCH][kVarRows], lvv[VCH][kVarRows], glv[VCH][kVarRows];
  auto chunk_load = [&](auto c0c) __attribute__((always_inline)) {
    constexpr int c0 = decltype(c0c)::value;
#pragma unroll
    for (int jj = 0; jj < VCH; jj++) {
      const int j = c0 + jj < NV ? c0 + jj : NV - 1;
#pragma unroll
      for (int u = 0; u < kVarRows; u++) {
        const int i = v.v_row(j, u);
        const int ii = i >= 0 ? i : 0;
        const bool general = v.v_poff(j, u) >= 0;
        tvv[jj][u] = tc[IDXL(ii)];
        lvv[jj][u] = lc[IDXL(ii)];
        glv[jj][u] = grow[IDXL(general ? ii : 0)];
      }
    }
  };
  auto chunk_rows = [&](auto c0c) __attribute__((always_inline)) {
    constexpr int c0 = decltype(c0c)::value;
#pragma unroll
    for (int jj = 0; jj < VCH; jj++) {
      const int j = c0 + jj;
      if (j >= NV) continue;
#pragma unroll
      for (int u = 0; u < kVarRows; u++) {
        const int i = v.v_row(j, u);
        if (i < 0) continue;
        sr.template var_row<V>(v, k, mu, j, u, z, dz, glv[jj][u], tvv[jj][u], lvv[jj][u]);
      }
    }
  };
  chunk_load(std::integral_constant<int, 0>{});
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (V::SPEC) {
    for_range<0, V::nfkrows()>([&](auto rc) __attribute__((always_inline)) { fk_row_body(decltype(rc)::value, fkin[decltype(rc)::value]); });
  } else {
    // (runtime tables: four rows' requests at a time, clamped to the last row; the row count is uniform)
    const int nfk = v.nfkrows();
    constexpr int FCH = NV <= 12 ? 4 : 1;
    for (int r0 = 0; r0 < nfk; r0 += FCH) {
      FkIn f4[FCH];
#pragma unroll
      for (int u = 0; u < FCH; u++) fk_load(r0 + u < nfk ? r0 + u : nfk - 1, f4[u]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < FCH; u++)
        if (r0 + u < nfk) fk_row_body(r0 + u, f4[u]);
    }
  }
  chunk_rows(std::integral_constant<int, 0>{});
  for_range<1, (NV + VCH - 1) / VCH>([&](auto cc) __attribute__((always_inline)) {
    constexpr int c0 = decltype(cc)::value * VCH;
    chunk_load(std::integral_constant<int, c0>{});
    __builtin_amdgcn_sched_barrier(0);
    chunk_rows(std::integral_constant<int, c0>{});
  });
  ap_out = sr.ap; ad_out = sr.ad; gphi_out = sr.gphi;
}

template <class C, class V>
__global__ __launch_bounds__(kSweepBlock) void k_step(const DevModel M, const DevTables *__restrict__ Tp, const Ws W,
                                              const int B) {
  const int gid = blockIdx.x * kSweepBlock + threadIdx.x;
  const int li = gid % W.Bp;
  const int k = __builtin_amdgcn_readfirstlane(gid / W.Bp);   // (uniform per wavefront, see k_sweep)
  if (li >= *W.n_act || k >= M.N) return;
  const int b = W.act_idx[li];
  if (W.status[b] != ST_ACTIVE || !W.newstep[b]) return;
  (void)B;
  const int cur = W.cur[b];
  StepIO<gdouble> io;
  io.zc = (gdouble *)W.z[cur]; io.tc = (gdouble *)W.t[cur]; io.lc = (gdouble *)W.lam[cur]; io.grow = (gdouble *)W.grow[cur];
  io.Jq = (gdouble *)W.Jq[cur]; io.dz = (gdouble *)W.dz; io.gfa = (gdouble *)W.gfa;
  io.SS = (size_t)M.N * W.Bp;
  io.loff = (unsigned)k * (unsigned)W.Bp + (unsigned)b;
  io.SSd = io.SS; io.loffd = io.loff;
  double ap, ad, gphi;
  const V v(M, *Tp);
  step_body<C, gdouble, V>(v, io, k, W.mu[b], ap, ad, gphi);
  // partial minima -> per-instance step lengths (min is order independent: deterministic)
  atomicMin(&W.amin_p[b], (unsigned long long)__double_as_longlong(ap));
  atomicMin(&W.amin_d[b], (unsigned long long)__double_as_longlong(ad));
  W.gphi[(size_t)k * W.Bp + b] = gphi;
}
