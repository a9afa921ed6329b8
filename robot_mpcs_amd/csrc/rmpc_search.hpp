// rmpc_search.hpp -- wide-window scan matching on the device, included by rmpc_world.hip behind
// rmpc_locate.hpp: the minimum pyramid of the edge-distance table (k_min_pyramid) and a branch-and-bound search of the
// lattice of rmpc_scan_match (k_scan_search; Olson 2009, the multi-resolution half).  Rotations are enumerated,
// translations branched.  A score is an int32 sum of table entries, a node's bound an int32 sum of pyramid entries that
// no candidate below it undercuts, and the choice the minimum of the strict order (score, m, k): the result is the
// exhaustive rule's bit for bit, whatever order the nodes are met in.  Contraction is off in every function here: the
// kernels evaluate the restatement's expressions (tests/scan_search_reference.py).

namespace rmpc {

constexpr int kSearchThreads = 256;
constexpr int kSearchMaxN = 127;        // nxy, nth <= 127: k < 255^3 < 2^24 and m <= 3 * 127^2 < 2^16
constexpr int kSearchMaxTop = 7;        // top_log2 <= 7: one top-level block of 128 x 128 covers half the widest lattice
constexpr int kSearchMaxLevels = 12;
constexpr int kSearchPop = 64;          // nodes expanded per round: 64 x 4 children, one per thread
// the node store, in LDS: one segment per height.  Nodes of height j < top_log2 are made only by a round that pops
// nodes of height j + 1, which happens only while no node of a height <= j is left: at most 4 x kSearchPop of them.
// Top-level nodes are taken in from the bound table in slices of kSearchThreads while fewer than kSearchPop wait.
constexpr int kSearchSeg = 4 * kSearchPop;
constexpr int kSearchTopSeg = kSearchPop + kSearchThreads;
constexpr int kSearchStore = kSearchTopSeg + (kSearchMaxTop - 1) * kSearchSeg;
static_assert(kSearchSeg == kSearchThreads, "k_scan_search: one child per thread");
static_assert(2 * kMatchMaxRays * sizeof(double) + kSearchStore * 2 * sizeof(int) <= 64 * 1024, "k_scan_search: LDS");

// Level l > 0 of the pyramid from level l - 1 (half = 2^(l - 1)): the least of the four windows of side half that tile
// the window of side 2 half at (R, C), those outside the map left out.  half = 0 copies d2 into level 0.
__global__ __launch_bounds__(256) void k_min_pyramid(const int *__restrict__ src, int *__restrict__ dst, int FH, int FW,
                                                     int half) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= FH * FW) return;
  const int R = g / FW, C = g - R * FW;
  int v = src[g];
  if (half > 0) {
    const bool right = C + half < FW, down = R + half < FH;
    if (right) v = min(v, src[g + half]);
    if (down) v = min(v, src[g + half * FW]);
    if (right && down) v = min(v, src[g + half * FW + half]);
  }
  dst[g] = v;
}

// the order (score, m, k) as the pair (score, m << 24 | k)
struct SearchKey {
  int score;
  unsigned long long mk;
};
__device__ __forceinline__ bool key_less(const SearchKey &a, const SearchKey &b) {
  return a.score < b.score || (a.score == b.score && a.mk < b.mk);
}
__device__ __forceinline__ SearchKey key_wave_min(SearchKey v) {
  for (int off = 32; off > 0; off >>= 1) {
    SearchKey o;
    o.score = __shfl_xor(v.score, off);
    o.mk = __shfl_xor(v.mk, off);
    if (key_less(o, v)) v = o;
  }
  return v;
}

// the least i^2 over i in [lo, hi]
__device__ __forceinline__ int least_square(int lo, int hi) {
  const int v = lo > 0 ? lo : hi < 0 ? -hi : 0;
  return v * v;
}

// what a node needs of the launch, read once per thread
struct SearchGeom {
  const int *d2, *pyr;
  double x, y, x0, y0, cell, sub, fw, fh, step_xy;
  int FW, FH, cap, levels, nxy, nth, nx, n;
};

// The node of rotation (c, s) and translations jx in [a, a1], jy in [b, b1] (include/rmpc.h, rmpc_scan_search).  A leaf
// (a == a1, b == b1, height 0) is scored by rule 4 of rmpc_scan_match.  Otherwise per used ray the fine columns at
// jx = a and a1 and the fine rows at jy = b and b1 bracket those of every candidate of the block (every operation of
// rules 3 and 4 is monotone in ix and in iy): the term is 0 when one of the four is not finite, cap when the bracket
// misses the map, and else the pyramid's entry at (Ra, Ca) of the least level whose window covers the bracket clipped
// into the map, 0 when that level was not built.  The lanes of a wave walk the rays together: one LDS word per ray.
__device__ __forceinline__ int search_node(const SearchGeom &g, const double *s_ux, const double *s_uy, double c, double s,
                                           int a, int a1, int b, int b1, bool leaf) {
#pragma clang fp contract(off)
  const double txa = g.x + (double)(a - g.nxy) * g.step_xy, txb = g.x + (double)(a1 - g.nxy) * g.step_xy;
  const double tya = g.y + (double)(b - g.nxy) * g.step_xy, tyb = g.y + (double)(b1 - g.nxy) * g.step_xy;
  int sum = 0;
  if (leaf) {
    for (int j = 0; j < g.n; j++) {
      const double ux = s_ux[j], uy = s_uy[j];
      const double qx = (c * ux - s * uy) + txa;
      const double qy = (s * ux + c * uy) + tya;
      const double ca = match_fine(qx, g.x0, g.cell, g.sub), ra = match_fine(qy, g.y0, g.cell, g.sub);
      int v = g.cap;
      if (ca >= 0.0 && ca < g.fw && ra >= 0.0 && ra < g.fh) v = g.d2[(int)ra * g.FW + (int)ca];
      sum += v;
    }
    return sum;
  }
  const size_t plane = (size_t)g.FH * g.FW;
  for (int j = 0; j < g.n; j++) {
    const double ux = s_ux[j], uy = s_uy[j];
    const double rx = c * ux - s * uy, ry = s * ux + c * uy;
    const double ca = match_fine(rx + txa, g.x0, g.cell, g.sub), cb = match_fine(rx + txb, g.x0, g.cell, g.sub);
    const double ra = match_fine(ry + tya, g.y0, g.cell, g.sub), rb = match_fine(ry + tyb, g.y0, g.cell, g.sub);
    int v = 0;
    if (isfinite(ca) && isfinite(cb) && isfinite(ra) && isfinite(rb)) {
      v = g.cap;
      if (!(cb < 0.0 || ca >= g.fw || rb < 0.0 || ra >= g.fh)) {
        const int Ca = (int)fmax(ca, 0.0), Cb = (int)fmin(cb, g.fw - 1.0);
        const int Ra = (int)fmax(ra, 0.0), Rb = (int)fmin(rb, g.fh - 1.0);
        const int e = max(Cb - Ca, Rb - Ra) + 1;                       // >= 1
        const int l = e <= 1 ? 0 : 32 - __clz(e - 1);                  // the least l with 2^l >= e
        v = l >= g.levels ? 0 : g.pyr[(size_t)l * plane + (size_t)Ra * g.FW + Ca];
      }
    }
    sum += v;
  }
  return sum;
}

// One workgroup per robot.  The used rays go into LDS as in k_scan_match.  Nodes are the words jth << 16 | by << 8 | bx
// with (bx, by) the block's position in units of its own side 2^height.
//  A. every top-level node is bounded, a thread a node, into the bound table (top_bound [b] when given, else the
//     robot's slice of work); at top_log2 = 0 these are the candidates' scores and their minimum is the result;
//  B. the incumbent: the top-level node least by (bound, m_min, index) is searched alone;
//  C. the other top-level nodes are taken in index order, in slices of 256, those whose key (bound, m_min, 0) is not
//     above the incumbent's are kept.  A round pops up to 64 nodes of the lowest height present, drops those whose key
//     has risen above the incumbent since, and gives each of the four children to a thread: a leaf is scored and
//     folded into the incumbent, any other child is bounded and, unless above the incumbent, stored one height down
//     (slots by ballot and popcount per wave, the waves' counts through LDS).
// A node is dropped only when its key is greater than the incumbent's full key (score, m, k), so every tie of
// (score, m) lives until k decides, and the store cannot overflow (kSearchStore above): nothing is ever lost.
__global__ __launch_bounds__(kSearchThreads) void k_scan_search(rmpc_scan_search m, int ntop, int nb) {
#pragma clang fp contract(off)
  __shared__ double s_ux[kMatchMaxRays], s_uy[kMatchMaxRays];
  __shared__ int s_node[kSearchStore], s_bound[kSearchStore];
  __shared__ int s_cnt[kSearchMaxTop + 1];
  __shared__ int s_wscore[kSearchThreads / 64], s_wn[kSearchThreads / 64];
  __shared__ unsigned long long s_wmk[kSearchThreads / 64];
  __shared__ int s_inc_score, s_n, s_leaves;
  __shared__ unsigned long long s_inc_mk;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, R = m.rays;
  const double *const p = m.pose + (size_t)b * m.pose_stride;
  const double x = p[0], y = p[1], th = p[2];
  if (tid == 0) { s_n = 0; s_leaves = 0; s_inc_score = INT_MAX; s_inc_mk = ~0ull; }
  if (tid <= kSearchMaxTop) s_cnt[tid] = 0;
  __syncthreads();
  for (int i = tid; i < R; i += kSearchThreads) {
    const size_t g = (size_t)b * R + i;
    const double t = m.ranges[g], px = m.points[3 * g], py = m.points[3 * g + 1];
    if (isfinite(t) && isfinite(px) && isfinite(py) && t > 0.0 && t < m.range) {
      const int slot = atomicAdd(&s_n, 1);
      s_ux[slot] = px - x;
      s_uy[slot] = py - y;
    }
  }
  __syncthreads();
  const int n = s_n;
  if (n < m.min_hits || (m.active && m.active[b] == 0)) {             // (the whole workgroup: both are uniform)
    if (tid == 0) {
      double *const o = m.pose_out + (size_t)b * 3;
      o[0] = x; o[1] = y; o[2] = th;
      m.best[b] = -1;
      m.score[b] = 0;
      if (m.score0) m.score0[b] = 0;
      if (m.used) m.used[b] = n;
      if (m.leaves) m.leaves[b] = 0;
    }
    return;
  }
  SearchGeom g;
  g.d2 = m.d2; g.pyr = m.pyr;
  g.x = x; g.y = y; g.x0 = m.x0; g.y0 = m.y0; g.cell = m.cell; g.sub = (double)m.sub; g.step_xy = m.step_xy;
  g.FW = m.W * m.sub; g.FH = m.H * m.sub; g.fw = (double)g.FW; g.fh = (double)g.FH;
  g.cap = m.cap; g.levels = m.levels; g.nxy = m.nxy; g.nth = m.nth; g.nx = 2 * m.nxy + 1; g.n = n;
  const int nx = g.nx, htop = m.top_log2;
  int *const tb = m.top_bound ? m.top_bound + (size_t)b * ntop : (int *)m.work + (size_t)b * ntop;
  int my_leaves = 0;

  // the key of the node (jth, bx, by) of height h and of the bound v; k only for a leaf
  const auto node_key = [&](int jth, int bx, int by, int h, int v) {
    const int a = bx << h, a1 = min(a + (1 << h), nx) - 1, c = by << h, c1 = min(c + (1 << h), nx) - 1;
    const int ith = jth - m.nth;
    const int mm = least_square(a - m.nxy, a1 - m.nxy) + least_square(c - m.nxy, c1 - m.nxy) + ith * ith;
    SearchKey k;
    k.score = v;
    k.mk = (unsigned long long)mm << 24 | (unsigned long long)(h == 0 ? (jth * nx + c) * nx + a : 0);
    return k;
  };
  const auto node_bound = [&](int jth, int bx, int by, int h) {
    const int a = bx << h, a1 = min(a + (1 << h), nx) - 1, c = by << h, c1 = min(c + (1 << h), nx) - 1;
    return search_node(g, s_ux, s_uy, m.rot[2 * jth], m.rot[2 * jth + 1], a, a1, c, c1, h == 0);
  };
  // the workgroup's least of `mine` into the incumbent (top-level nodes: into s_w* [0] alone, with fold = false)
  const auto fold_min = [&](SearchKey mine, bool fold) {
    mine = key_wave_min(mine);
    if (lane == 0) { s_wscore[wave] = mine.score; s_wmk[wave] = mine.mk; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kSearchThreads / 64; w++) {
        SearchKey o;
        o.score = s_wscore[w]; o.mk = s_wmk[w];
        if (key_less(o, mine)) mine = o;
      }
      SearchKey inc;
      inc.score = s_inc_score; inc.mk = s_inc_mk;
      if (fold && key_less(mine, inc)) { s_inc_score = mine.score; s_inc_mk = mine.mk; }
      s_wscore[0] = mine.score; s_wmk[0] = mine.mk;
    }
    __syncthreads();
  };

  // A. the top level
  int score0 = 0;                                                     // (thread 0's: the centre candidate)
  if (tid == 0)
    score0 = search_node(g, s_ux, s_uy, m.rot[2 * m.nth], m.rot[2 * m.nth + 1], m.nxy, m.nxy, m.nxy, m.nxy, true);
  SearchKey mine;
  mine.score = INT_MAX; mine.mk = ~0ull;
  for (int t = tid; t < ntop; t += kSearchThreads) {
    const int bx = t % nb, by = (t / nb) % nb, jth = t / (nb * nb);
    const int v = node_bound(jth, bx, by, htop);
    tb[t] = v;
    SearchKey k = node_key(jth, bx, by, htop, v);
    if (htop == 0) my_leaves++;
    else k.mk |= (unsigned long long)t;                               // the least top-level node: ties by its index
    if (key_less(k, mine)) mine = k;
  }
  fold_min(mine, htop == 0);                                         // (also orders tb before what follows)
  const int t_first = htop == 0 ? -1 : (int)(s_wmk[0] & 0xffffffull);

  // B and C
  int next = 0;
  bool first = true, slices = false;                                  // no slice before the first node is searched out
  while (htop > 0) {
    __syncthreads();
    SearchKey inc;
    inc.score = s_inc_score; inc.mk = s_inc_mk;
    int h = 1;
    while (h <= htop && s_cnt[h] == 0) h++;
    if (first) {                                                      // B: the store holds the least node alone
      if (tid == 0) {
        s_node[0] = (t_first / (nb * nb)) << 16 | ((t_first / nb) % nb) << 8 | t_first % nb;
        s_bound[0] = tb[t_first];
        s_cnt[htop] = 1;
      }
      first = false;
      continue;
    }
    slices = slices || h > htop;
    if (slices && (h > htop || (h == htop && s_cnt[htop] < kSearchPop)) && next < ntop) {   // C: take a slice in
      const int t = next + tid;
      bool keep = false;
      int word = 0, v = 0;
      if (t < ntop && t != t_first) {
        const int bx = t % nb, by = (t / nb) % nb, jth = t / (nb * nb);
        v = tb[t];
        word = jth << 16 | by << 8 | bx;
        keep = !key_less(inc, node_key(jth, bx, by, htop, v));
      }
      const unsigned long long bal = __ballot(keep);
      if (lane == 0) s_wn[wave] = __popcll(bal);
      __syncthreads();
      int at = s_cnt[htop] + __popcll(bal & ((1ull << lane) - 1ull));
      for (int w = 0; w < wave; w++) at += s_wn[w];
      if (keep) { s_node[at] = word; s_bound[at] = v; }
      __syncthreads();
      if (tid == 0) s_cnt[htop] += s_wn[0] + s_wn[1] + s_wn[2] + s_wn[3];
      next += kSearchThreads;
      continue;
    }
    if (h > htop) break;
    // a round: the last `take` nodes of height h, four children each
    const int base = h == htop ? 0 : kSearchTopSeg + (h - 1) * kSearchSeg;
    const int have = s_cnt[h], take = min(have, kSearchPop), par = tid >> 2;
    const int hc = h - 1, basec = hc == 0 ? 0 : kSearchTopSeg + (hc - 1) * kSearchSeg;
    bool live = false;
    int jth = 0, bx = 0, by = 0;
    if (par < take) {
      const int word = s_node[base + have - 1 - par], v = s_bound[base + have - 1 - par];
      jth = word >> 16;
      live = !key_less(inc, node_key(jth, word & 255, (word >> 8) & 255, h, v));
      bx = 2 * (word & 255) + (tid & 1);
      by = 2 * ((word >> 8) & 255) + ((tid >> 1) & 1);
      live = live && (bx << hc) < nx && (by << hc) < nx;
    }
    int v = 0;
    SearchKey k;
    k.score = INT_MAX; k.mk = ~0ull;
    if (live) {
      v = node_bound(jth, bx, by, hc);
      k = node_key(jth, bx, by, hc, v);
    }
    __syncthreads();                                                  // every parent is read: its slots may be reused
    if (hc == 0) {
      if (live) my_leaves++;
      if (tid == 0) s_cnt[h] = have - take;
      fold_min(k, true);
    } else {
      const bool keep = live && !key_less(inc, k);
      const unsigned long long bal = __ballot(keep);
      if (lane == 0) s_wn[wave] = __popcll(bal);
      __syncthreads();
      int at = basec + __popcll(bal & ((1ull << lane) - 1ull));       // (height hc is empty: h is the lowest present)
      for (int w = 0; w < wave; w++) at += s_wn[w];
      if (keep) { s_node[at] = jth << 16 | by << 8 | bx; s_bound[at] = v; }
      if (tid == 0) { s_cnt[h] = have - take; s_cnt[hc] = s_wn[0] + s_wn[1] + s_wn[2] + s_wn[3]; }
    }
  }
  if (m.leaves) atomicAdd(&s_leaves, my_leaves);
  __syncthreads();
  if (tid == 0) {
    const int k = (int)(s_inc_mk & 0xffffffull);
    const int jx = k % nx, jy = (k / nx) % nx, jth = k / (nx * nx);
    double *const o = m.pose_out + (size_t)b * 3;
    o[0] = x + (double)(jx - m.nxy) * m.step_xy;
    o[1] = y + (double)(jy - m.nxy) * m.step_xy;
    o[2] = th + (double)(jth - m.nth) * m.step_th;
    m.best[b] = k;
    m.score[b] = s_inc_score;
    if (m.score0) m.score0[b] = score0;
    if (m.used) m.used[b] = n;
    if (m.leaves) m.leaves[b] = s_leaves;
  }
}

}  // namespace rmpc
