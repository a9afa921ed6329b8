// rmpc_ecbs.hpp -- bounded-suboptimal timed routes: focal conflict-based search on the device (include/rmpc_ecbs.h,
// DESIGN.md 32), included by rmpc_world.hip behind rmpc_cbs.hpp.  The rule is written out in the header; here are its
// three kernels, in the stream discipline of rmpc_cbs.hpp: the host enqueues root, `rounds` x (select, expand) and the
// report blind, a kernel behind a stop returns on the header's flag, and what a kernel reads of other workgroups was
// written by an earlier kernel of the stream.
//
//  k_ecbs_root    one workgroup: the free mask, every robot's focal route under the empty table, node 0.
//  k_ecbs_select  one workgroup, once per round and once more as the report: one pass over the ids in use finds the
//                 incumbent, Lo and the best open node and decides rules 1 and 2; a second pass takes the e least of
//                 FOCAL at once -- every thread keeps the kEcbsKeep least keys of its ids in LDS, and the heads of the
//                 256 lists are merged; a further pass is needed only when one thread held more than kEcbsKeep of them.
//  k_ecbs_expand  one workgroup per child, 2 E per round: the child's table, the shortest route of the constrained robot
//                 (timed_robot, which leaves reach[0 .. T] in the history), then the focal route on those layers
//                 (ecbs_focal), the parent's other paths, the node's conflict and the number of its conflicts.
//
// What is taken from rmpc_cbs.hpp and rmpc_timed.hpp is called as it stands (timed_robot, cbs_constrain, cbs_block_min,
// cbs_clear_table, CbsHdr): nothing there is changed or given a new template argument, so the kernels of those headers
// come out as they were.  The conflict scan is a copy with a count beside the key.
//
// The workspace: CbsHdr, the free mask, per node its conflict key, then the slots, then per node parent, constraint,
// cost, state, lb, nconf, the robots' arrive, lbs and paths as int16.  A slot is what rmpc_cbs.hpp's is (table, history,
// int32 path), then one byte per (t, cell) -- the origin the layer recursion chose, so that the backtrack reads no costs
// -- and three int32 rows of cells (two cost rows, the penalty layer), used when the rows do not fit in LDS.

#include <climits>
#include <cstdint>

namespace rmpc {

constexpr int kEcbsBig = 1 << 30;                 // a cost no cell of a layer has
constexpr int kEcbsRowsLds = 40 * 1024;           // the three rows of a route live in LDS up to this size (H W <= 3413)
constexpr int kEcbsKeep = 2;                      // keys a thread of k_ecbs_select keeps per pass
constexpr int kEcbsWin = 2 * RMPC_TIMED_MAX_LAG + 2;

// byte offsets into the workspace and the words of a slot.  The six int32 arrays of the nodes lie one behind the other
// from `node`, m4 bytes each, the two int16 arrays of the robots behind them, mb2 bytes each, then the paths: few
// members, because every kernel holds them in scalar registers throughout.
struct EcbsLayout {
  long long conf, slots, node, m4, mb2, total;
  long long slot_words, dir_word, row_word;      // a slot, and where its origins and cost rows begin, in 8-byte words
};

__host__ static inline EcbsLayout ecbs_layout(int H, int W, int T, int B, int M, int E) {
  const long long L = (long long)H * ((W + 63) / 64), HW = (long long)H * W;
  EcbsLayout y;
  y.dir_word = timed_order_words(H, W, T) + (T + 2) / 2;
  y.row_word = y.dir_word + ((long long)(T + 1) * HW + 7) / 8;
  y.slot_words = y.row_word + (3 * HW + 1) / 2;
  y.conf = (long long)sizeof(CbsHdr) + 8 * L;                  // (the free mask lies behind the header)
  y.slots = y.conf + 8LL * M;
  y.node = y.slots + 8 * y.slot_words * 2 * E;
  y.m4 = 4LL * M;
  y.mb2 = 2LL * M * B;
  y.total = y.node + 6 * y.m4 + 2 * y.mb2 + y.mb2 * (T + 1);
  y.total = (y.total + 7) / 8 * 8;
  return y;
}

struct EcbsPool {
  char *w;
  const EcbsLayout &y;
  __device__ __forceinline__ CbsHdr *hdr() const { return (CbsHdr *)w; }
  __device__ __forceinline__ timed_word *freeb() const { return (timed_word *)(w + sizeof(CbsHdr)); }
  __device__ __forceinline__ timed_word *slots() const { return (timed_word *)(w + y.slots); }
  __device__ __forceinline__ unsigned long long *conf() const { return (unsigned long long *)(w + y.conf); }
  __device__ __forceinline__ int *parent() const { return (int *)(w + y.node); }
  __device__ __forceinline__ int *con() const { return (int *)(w + y.node + y.m4); }
  __device__ __forceinline__ int *cost() const { return (int *)(w + y.node + 2 * y.m4); }
  __device__ __forceinline__ int *state() const { return (int *)(w + y.node + 3 * y.m4); }
  __device__ __forceinline__ int *lb() const { return (int *)(w + y.node + 4 * y.m4); }
  __device__ __forceinline__ int *nconf() const { return (int *)(w + y.node + 5 * y.m4); }
  __device__ __forceinline__ short *arrive() const { return (short *)(w + y.node + 6 * y.m4); }
  __device__ __forceinline__ short *lbs() const { return (short *)(w + y.node + 6 * y.m4 + y.mb2); }
  __device__ __forceinline__ short *paths() const { return (short *)(w + y.node + 6 * y.m4 + 2 * y.mb2); }
};

__device__ __forceinline__ bool ecbs_skipped(const rmpc_ecbs &p, int b) {
  const int s = p.start_cell[b], gi = p.goal_index[b];
  return s < 0 || s >= p.H * p.W || gi < 0 || gi >= p.Gf;
}

// the static LDS of a workgroup that routes
struct EcbsLds {
  unsigned long long red_k[kTimedThreads];
  int red_c[kTimedThreads];
  int raw[RMPC_TIMED_MAX_T + 1];                   // pen[v][g]
  int cand[RMPC_TIMED_MAX_T + 1];                  // per arrival a2: (the least c[a2 - 1][g - move] << 4) | move
  int win[kEcbsWin * RMPC_CBS_MAX_ROBOTS];         // the others' cells (row << 16 | col) in the layers around t
  int oj[RMPC_CBS_MAX_ROBOTS];                     // the robots of O
  int sa[2], n_o;
};

// the slot of a workgroup as timed_robot wants it, with the one free mask the root made
template <bool kLds>
__device__ __forceinline__ TimedWork ecbs_slot(const EcbsPool &pool, int slot, const TimedGeom &q, int T) {
  TimedWork wk = timed_work_at<kLds>(pool.slots(), slot, q, T);
  wk.freeb = pool.freeb();
  return wk;
}

// the node's conflict key as cbs_conflict forms it, and the number of its conflicts
struct EcbsConflict {
  unsigned long long key;
  int count;
};

// ends behind a barrier
__device__ __forceinline__ EcbsConflict ecbs_conflict(const short *paths, int B, int T, int W, int sep2, int lag,
                                                      unsigned long long *red, int *red_c, int tid, int nt) {
  unsigned long long best = kCbsNoKey;
  int n_c = 0;
  const int T1 = T + 1;
  for (int i = 0; i < B - 1; i++) {
    const short *const pi = paths + (size_t)i * T1;
    if (pi[0] < 0) continue;                                   // skipped (uniform)
    const int n = (B - 1 - i) * T1;
    for (int it = tid; it < n; it += nt) {
      const int dj = it / T1, t = it - dj * T1, j = i + 1 + dj;
      const short *const pj = paths + (size_t)j * T1;
      if (pj[0] < 0) continue;
      const int ci = pi[t], ri = ci / W, coli = ci - ri * W;
      const int s0 = t - lag > 0 ? t - lag : 0, s1 = t + lag < T ? t + lag : T;
      for (int s = s0; s <= s1; s++) {
        if ((t | s) == 0) continue;
        const int cj = pj[s], dr = cj / W - ri, dc = cj % W - coli;
        if (dr * dr + dc * dc < sep2) {
          const unsigned long long key = ((unsigned long long)(t < s ? t : s) << 32) | ((unsigned long long)i << 26) |
                                         ((unsigned long long)j << 20) | ((unsigned long long)t << 10) | (unsigned long long)s;
          best = key < best ? key : best;
          n_c++;
        }
      }
    }
  }
  red_c[tid] = n_c;
  __syncthreads();
  for (int h = nt >> 1; h > 0; h >>= 1) {
    if (tid < h) red_c[tid] += red_c[tid + h];
    __syncthreads();
  }
  const int count = red_c[0];
  return {cbs_block_min(best, red, tid, nt), count};           // (its first barrier is behind every read of red_c[0])
}

// A word of the penalty layer.  In LDS (kRows) it is read and written as it stands; in the workspace the adds are atomics
// that settle in L2, so the reads and the clearing stores go there as well and no reader is served a line from before them.
template <bool kRows>
__device__ __forceinline__ int ecbs_pen_load(const int *p) {
  return kRows ? *p : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool kRows>
__device__ __forceinline__ void ecbs_pen_store(int *p, int v) {
  if (kRows) *p = v;
  else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The FOCAL ROUTE of robot b on the layers reach[0 .. T] that timed_robot left in hist, against the robots j < jmax,
// j != b of opaths [B][T + 1] that are not skipped: path32 holds the shortest path p with the least arrive a (uniform) and
// is left holding the focal path; returns its arrive a2 (uniform).  rows: three int32 rows of H W (two cost rows and
// the penalty layer); dirs: (T + 1) H W bytes.
// Called by the whole workgroup under uniform control flow; ends behind a barrier.
template <bool kRows>
__device__ __forceinline__ int ecbs_focal(const TimedDims &d, const timed_word *hist, int *__restrict__ path32, int a, int g,
                                          const short *__restrict__ opaths, int b, int jmax, int w_num, int w_den,
                                          int *rows, unsigned char *__restrict__ dirs, EcbsLds &s) {
  const int H = d.H, W = d.W, HW = H * W, T = d.T, T1 = T + 1, lag = d.lag, sep2 = d.sep2, tid = d.tid, nt = d.nt;
  if (a == 0 || a == T + 1) return a;                          // the path stands on g throughout, or never holds it: p
  const long long wa = (long long)w_num * a / w_den;
  const int A = wa < T ? (int)wa : T;
  const int nl = 2 * lag + 2;
  const int gr = g / W, gc = g - gr * W;

  if (tid == 0) {
    int n = 0;
    for (int j = 0; j < jmax; j++)
      if (j != b && opaths[(size_t)j * T1] >= 0) s.oj[n++] = j;
    s.n_o = n;
  }
  __syncthreads();
  const int n_o = s.n_o;
  // pen[v][g] for every layer, from the paths themselves
  for (int v = tid; v <= T; v += nt) {
    int n = 0;
    const int s0 = v - lag > 0 ? v - lag : 0, s1 = v + lag < T ? v + lag : T;
    for (int k = 0; k < n_o; k++) {
      const short *const pj = opaths + (size_t)s.oj[k] * T1;
      for (int u = s0; u <= s1; u++) {
        if ((v | u) == 0) continue;
        const int cj = pj[u], dr = cj / W - gr, dc = cj % W - gc;
        n += dr * dr + dc * dc < sep2;
      }
    }
    s.raw[v] = n;
  }
  // the window's first layers 0 .. lag, and an empty penalty layer
  for (int i = tid; i < (lag + 1) * n_o; i += nt) {
    const int u = i / n_o, k = i - u * n_o;
    if (u <= T) {
      const int cj = opaths[(size_t)s.oj[k] * T1 + u];
      s.win[(u % nl) * RMPC_CBS_MAX_ROBOTS + k] = ((cj / W) << 16) | (cj % W);
    }
  }
  int *const pen = rows + 2 * (size_t)HW;
  for (int x = tid; x < HW; x += nt) ecbs_pen_store<kRows>(pen + x, 0);
  __syncthreads();

  // pen += sign on the cells that conflict with the cells of O in layer u of the window: one (robot, disc row) per thread
  // and pass, atomic adds because the discs of two robots overlap
  const int side = 2 * d.rad + 1;
  const int *const win = s.win;                                // (a copy of s in the closure would be 14 KB per lane)
  const auto stamp = [=](int u, int sign) {
    const int *const wl = win + (u % nl) * RMPC_CBS_MAX_ROBOTS;
    for (int i = tid; i < n_o * side; i += nt) {
      const int k = i / side, dr = i - k * side - d.rad;
      const int wv = wl[k], r = (wv >> 16) + dr, col = wv & 0xffff;
      if (r < 0 || r >= H) continue;
      const int h = timed_half_width(dr, d.rad, sep2);
      const int lo = col - h > 0 ? col - h : 0, hi = col + h < W - 1 ? col + h : W - 1;
      for (int c = lo; c <= hi; c++) atomicAdd(pen + r * W + c, sign);
    }
  };
  for (int u = 1; u <= lag && u <= T; u++) stamp(u, 1);           // pen[0]: layer 0 of O is exempt
  __syncthreads();

  // the least c[t - 1][g - move] over the moves, with the first move that attains it (one thread)
  const auto candidate = [=](const int *prev) {
    int best = INT_MAX;
    for (int m = 0; m < d.movement; m++) {
      const int rr = gr - grid_dr(m), cc = gc - grid_dc(m);
      if (rr < 0 || rr >= H || cc < 0 || cc >= W) continue;
      const int v = prev[rr * W + cc];
      if (v < kEcbsBig && ((v << 4) | m) < best) best = (v << 4) | m;       // (v rises before m does)
    }
    return best;
  };

  // The layer recursion: one thread per cell, row t from row t - 1.  The penalty layer is carried from pen[t - 1] to
  // pen[t] by the discs of O's layer that enters the window (t + lag; at t = 1 layer 0 too) and of the one that leaves it
  // (t - lag - 1), then a barrier, then the row, then the layer's barrier.  The window's layer t + lag + 1 is fetched
  // under row t: its place is the one of layer t - lag - 1, whose discs were taken out before the first barrier.
  for (int t = 0; t < A; t++) {
    int *const cur = rows + (size_t)(t & 1) * HW;
    const int *const prev = rows + (size_t)((t & 1) ^ 1) * HW;
    if (t >= 1) {
      if (t + lag <= T) stamp(t + lag, 1);
      if (t == 1) stamp(0, 1);
      if (t - lag - 1 >= 0) stamp(t - lag - 1, -1);
      __syncthreads();
    }
    const int u_new = t + lag + 1;
    if (u_new <= T)
      for (int k = tid; k < n_o; k += nt) {
        const int cj = opaths[(size_t)s.oj[k] * T1 + u_new];
        s.win[(u_new % nl) * RMPC_CBS_MAX_ROBOTS + k] = ((cj / W) << 16) | (cj % W);
      }
    if (t >= a && tid == nt - 1) s.cand[t] = candidate(prev);
    const timed_word *const layer = hist + (size_t)t * d.L;
    for (int x = tid; x < HW; x += nt) {
      const int r = x / W, col = x - r * W;
      int v = kEcbsBig;
      if (timed_bit(layer, d.Wd, r, col)) {
        int best = 0, from = 0;
        if (t > 0) {
          best = prev[x];
          for (int m = 0; m < d.movement; m++) {
            const int rr = r - grid_dr(m), cc = col - grid_dc(m);
            if (rr < 0 || rr >= H || cc < 0 || cc >= W) continue;
            const int pv = prev[rr * W + cc];
            if (pv < best) { best = pv; from = m + 1; }
          }
        }
        v = best + ecbs_pen_load<kRows>(pen + x);
        dirs[(size_t)t * HW + x] = (unsigned char)from;
      }
      cur[x] = v;
    }
    __syncthreads();
  }
  if (tid == nt - 1) s.cand[A] = candidate(rows + (size_t)((A - 1) & 1) * HW);
  __syncthreads();

  // the arrival: the least (total, a2), the first move behind it
  unsigned long long key = kCbsNoKey;
  for (int a2 = a + tid; a2 <= A; a2 += nt) {
    const int cv = s.cand[a2];
    if (cv == INT_MAX) continue;
    int hold = 0;
    for (int v = a2; v <= T; v++) hold += s.raw[v];
    const unsigned long long k2 = ((unsigned long long)((cv >> 4) + hold) << 32) | ((unsigned long long)a2 << 4) | (unsigned)(cv & 15);
    key = k2 < key ? k2 : key;
  }
  key = cbs_block_min(key, s.red_k, tid, nt);
  const int a2 = (int)((key >> 4) & 0xfffffff), m = (int)(key & 15);
  for (int t = a2 + tid; t <= T; t += nt) path32[t] = g;
  if (tid == 0) {
    int r = gr - grid_dr(m), col = gc - grid_dc(m);
    path32[a2 - 1] = r * W + col;
    for (int t = a2 - 1; t > 0; t--) {
      const int from = dirs[(size_t)t * HW + r * W + col];
      if (from) { r -= grid_dr(from - 1); col -= grid_dc(from - 1); }
      path32[t - 1] = r * W + col;
    }
  }
  __syncthreads();
  return a2;
}

// where the three rows of a workgroup live: behind the history in LDS, or in its slot
template <bool kLds, bool kRows>
__device__ __forceinline__ int *ecbs_rows(const TimedWork &wk, const EcbsLayout &y, const TimedGeom &q, int T) {
  extern __shared__ timed_word timed_lds[];
  return kRows ? (int *)(timed_lds + (kLds ? (size_t)(T + 1) * q.L : 0)) : (int *)(wk.res + y.row_word);
}

template <bool kLds, bool kRows>
__global__ __launch_bounds__(kTimedThreads) void k_ecbs_root(rmpc_ecbs p, TimedGeom q, EcbsLayout y, int magic) {
  __shared__ EcbsLds s;
  const int tid = threadIdx.x, nt = blockDim.x, B = p.B, T = p.T;
  const TimedDims d = {p.H, p.W, q.Wd, q.L, T, p.lag, p.sep2, q.rad, p.movement, tid, nt};
  const EcbsPool pool = {(char *)p.work, y};
  const TimedWork wk = ecbs_slot<kLds>(pool, 0, q, T);
  int *const path32 = (int *)(wk.res + (y.dir_word - (T + 2) / 2));
  unsigned char *const dirs = (unsigned char *)(wk.res + y.dir_word);
  int *const rows = ecbs_rows<kLds, kRows>(wk, y, q, T);
  timed_free_mask(pool.freeb(), p.grid, p.occ_threshold, d);
  cbs_clear_table(wk, d);
  __syncthreads();
  TimedNoStartRule rule;
  bool dead = false;
  int cost = 0, lb = 0;                                        // thread 0's
  for (int b = 0; b < B; b++) {
    short *const path = pool.paths() + (size_t)b * (T + 1);
    if (ecbs_skipped(p, b)) {
      for (int t = tid; t <= T; t += nt) path[t] = -1;
      if (tid == 0) { pool.arrive()[b] = pool.lbs()[b] = (short)(T + 1); cost += T + 1; lb += T + 1; }
      continue;
    }
    const TimedEnd e = timed_robot<false, false>(d, wk, rule, p.fields, p.goal_cells, p.start_cell[b], 0, 0, nullptr,
                                                 p.goal_index[b], 0, path32, nullptr, s.sa, s.sa + 1, (double *)s.red_k, s.red_c);
    if (e.f) { dead = true; break; }                           // (uniform)
    const int a = s.sa[1];
    const int a2 = ecbs_focal<kRows>(d, wk.hist, path32, a, p.goal_cells[p.goal_index[b]], pool.paths(), b, b, p.w_num, p.w_den,
                              rows, dirs, s);
    for (int t = tid; t <= T; t += nt) path[t] = (short)path32[t];
    if (tid == 0) { pool.arrive()[b] = (short)a2; pool.lbs()[b] = (short)a; cost += a2; lb += a; }
    __syncthreads();                                           // path32 and sa are read before the next robot writes them
  }
  EcbsConflict c = {kCbsNoKey, 0};
  if (!dead) {
    __syncthreads();
    c = ecbs_conflict(pool.paths(), B, T, p.W, p.sep2, p.lag, s.red_k, s.red_c, tid, nt);
  }
  const unsigned long long key = c.key;
  const int n_c = c.count;
  if (tid == 0) {
    CbsHdr *const h = pool.hdr();
    h->magic = magic; h->stop = 0; h->expanded = 0; h->x0 = 0; h->n_take = 0; h->rounds_run = 0; h->created = dead ? 0 : 1;
    pool.parent()[0] = -1; pool.con()[0] = 0; pool.cost()[0] = cost; pool.lb()[0] = lb; pool.nconf()[0] = n_c;
    pool.conf()[0] = key;
    pool.state()[0] = dead ? kCbsNone : (key == kCbsNoKey ? kCbsSolution : kCbsOpen);
  }
}

template <bool kLds, bool kRows>
__global__ __launch_bounds__(kTimedThreads) void k_ecbs_expand(rmpc_ecbs p, TimedGeom q, EcbsLayout y) {
  __shared__ EcbsLds s;
  const int tid = threadIdx.x, nt = blockDim.x, B = p.B, T = p.T, T1 = T + 1;
  const EcbsPool pool = {(char *)p.work, y};
  const CbsHdr *const h = pool.hdr();
  if (h->stop != 0 || (int)blockIdx.x >= 2 * h->n_take) return;          // (the select kernel of this round wrote both)
  const int k = blockIdx.x >> 1, which = blockIdx.x & 1;
  const int parent = h->take[k], id = 1 + 2 * (h->x0 + k) + which;
  const unsigned long long ck = pool.conf()[parent];
  const int ci = (int)(ck >> 26) & 63, cj = (int)(ck >> 20) & 63, ct = (int)(ck >> 10) & 1023, cs = (int)ck & 1023;
  const short *const ppaths = pool.paths() + (size_t)parent * B * T1;
  if ((which == 0 ? ct : cs) < 1) {                            // the child does not exist
    if (tid == 0) pool.state()[id] = kCbsNone;
    return;
  }
  const int r = which == 0 ? ci : cj;
  const int con = cbs_con(which, r, cs, ppaths[(size_t)cj * T1 + cs]);

  const TimedDims d = {p.H, p.W, q.Wd, q.L, T, p.lag, p.sep2, q.rad, p.movement, tid, nt};
  const TimedWork wk = ecbs_slot<kLds>(pool, blockIdx.x, q, T);
  int *const path32 = (int *)(wk.res + (y.dir_word - (T + 2) / 2));
  unsigned char *const dirs = (unsigned char *)(wk.res + y.dir_word);
  int *const rows = ecbs_rows<kLds, kRows>(wk, y, q, T);
  cbs_clear_table(wk, d);
  __syncthreads();
  cbs_constrain(wk.res, con, d);
  for (int n = parent; n > 0; n = pool.parent()[n]) {            // the chain to the root (uniform: scalar loads)
    const int c = pool.con()[n];
    if (((c >> 24) & 63) == r) cbs_constrain(wk.res, c, d);
  }
  __syncthreads();
  TimedNoStartRule rule;
  const TimedEnd e = timed_robot<false, false>(d, wk, rule, p.fields, p.goal_cells, p.start_cell[r], 0, 0, nullptr,
                                               p.goal_index[r], 0, path32, nullptr, s.sa, s.sa + 1, (double *)s.red_k, s.red_c);
  if (e.f) {                                                   // the route does not exist: the child is dead
    if (tid == 0) pool.state()[id] = kCbsNone;
    return;
  }
  const int a = s.sa[1];
  const int a2 = ecbs_focal<kRows>(d, wk.hist, path32, a, p.goal_cells[p.goal_index[r]], ppaths, r, B, p.w_num, p.w_den, rows, dirs, s);
  short *const paths = pool.paths() + (size_t)id * B * T1;
  for (int i = tid; i < B * T1; i += nt) {
    const int b = i / T1;
    paths[i] = b == r ? (short)path32[i - b * T1] : ppaths[i];
  }
  for (int b = tid; b < B; b += nt) {
    pool.arrive()[(size_t)id * B + b] = b == r ? (short)a2 : pool.arrive()[(size_t)parent * B + b];
    pool.lbs()[(size_t)id * B + b] = b == r ? (short)a : pool.lbs()[(size_t)parent * B + b];
  }
  __syncthreads();
  const EcbsConflict c = ecbs_conflict(paths, B, T, p.W, p.sep2, p.lag, s.red_k, s.red_c, tid, nt);
  const unsigned long long key = c.key;
  const int n_c = c.count;
  if (tid == 0) {
    pool.parent()[id] = parent; pool.con()[id] = con; pool.conf()[id] = key;
    pool.cost()[id] = pool.cost()[parent] - (int)pool.arrive()[(size_t)parent * B + r] + a2;
    pool.lb()[id] = pool.lb()[parent] - (int)pool.lbs()[(size_t)parent * B + r] + a;
    pool.nconf()[id] = n_c;
    pool.state()[id] = key == kCbsNoKey ? kCbsSolution : kCbsOpen;
    atomicAdd(&pool.hdr()->created, 1);
  }
}

// a node's place in FOCAL's order: (nconf, cost, id) in 25, 17 and 21 bits
__device__ __forceinline__ unsigned long long ecbs_rank(int nconf, int cost, int id) {
  return ((unsigned long long)(unsigned)nconf << 38) | ((unsigned long long)(unsigned)cost << 21) | (unsigned)id;
}

// One round's decision, or with `report` the outputs.  `first`: the first kernel of a call that reads the header -- it
// checks that the workspace holds a search of these arguments and takes no earlier stop for its own.
__global__ __launch_bounds__(256) void k_ecbs_select(rmpc_ecbs p, EcbsLayout y, int magic, int first, int report) {
  __shared__ unsigned long long red_k[256];
  __shared__ unsigned long long lst[kEcbsKeep * 256];
  __shared__ int takes[RMPC_CBS_MAX_EXPAND];
  const int tid = threadIdx.x, B = p.B, T = p.T, T1 = T + 1;
  const EcbsPool pool = {(char *)p.work, y};
  CbsHdr *const h = pool.hdr();
  const bool bad = h->magic != magic;
  const int stop = first ? (bad ? RMPC_CBS_BAD_STATE : 0) : h->stop;
  __syncthreads();                                             // every thread has read the flag before thread 0 sets it
  if (stop != 0 && !report) {
    if (first && tid == 0) { h->stop = stop; h->n_take = 0; }
    return;
  }
  // the incumbent by (cost, id), the best open node by (nconf, cost, id), Lo over both kinds
  unsigned long long inc = kCbsNoKey, opn = kCbsNoKey, lo = kCbsNoKey;
  const int expanded = bad ? 0 : h->expanded;
  const int hi = 1 + 2 * expanded;
  if (!bad) {
    unsigned long long mi = kCbsNoKey, mo = kCbsNoKey, ml = kCbsNoKey;
    for (int id = tid; id < hi; id += 256) {
      const int st = pool.state()[id];
      if (st != kCbsOpen && st != kCbsSolution) continue;
      const int cost = pool.cost()[id];
      const unsigned long long l = (unsigned)pool.lb()[id];
      ml = l < ml ? l : ml;
      if (st == kCbsOpen) {
        const unsigned long long key = ecbs_rank(pool.nconf()[id], cost, id);
        mo = key < mo ? key : mo;
      } else {
        const unsigned long long key = ((unsigned long long)(unsigned)cost << 32) | (unsigned)id;
        mi = key < mi ? key : mi;
      }
    }
    inc = cbs_block_min(mi, red_k, tid, 256);
    opn = cbs_block_min(mo, red_k, tid, 256);
    lo = cbs_block_min(ml, red_k, tid, 256);
  }
  const int inc_cost = inc == kCbsNoKey ? RMPC_CBS_INF : (int)(inc >> 32);
  const int lo_lb = lo == kCbsNoKey ? RMPC_CBS_INF : (int)lo;

  if (report) {
    const int node = inc != kCbsNoKey ? (int)(unsigned)inc : (opn != kCbsNoKey ? (int)(opn & 0x1fffff) : -1);
    if (tid == 0) {
      if (first) h->stop = stop;
      int *const o = p.info;
      o[RMPC_CBS_OUTCOME] = stop ? stop : RMPC_CBS_ROUNDS;
      o[RMPC_CBS_NODE] = node;
      o[RMPC_CBS_CONFLICT_FREE] = inc != kCbsNoKey;
      o[RMPC_CBS_COST] = node < 0 ? RMPC_CBS_INF : pool.cost()[node];
      o[RMPC_CBS_BOUND] = lo_lb;
      o[RMPC_CBS_CREATED] = bad ? 0 : h->created;
      o[RMPC_CBS_EXPANDED] = expanded;
      o[RMPC_CBS_ROUNDS_RUN] = bad ? 0 : h->rounds_run;
      o[RMPC_ECBS_LB] = node < 0 ? RMPC_CBS_INF : pool.lb()[node];
      o[RMPC_ECBS_NCONF] = node < 0 ? 0 : pool.nconf()[node];
    }
    for (int i = tid; i < B * T1; i += 256) p.paths[i] = node < 0 ? -1 : (int)pool.paths()[(size_t)node * B * T1 + i];
    for (int b = tid; b < B; b += 256) {
      p.arrive[b] = node < 0 ? T + 1 : (int)pool.arrive()[(size_t)node * B + b];
      p.status[b] = ecbs_skipped(p, b) ? RMPC_GRID_OUTSIDE : 0;
    }
    return;
  }

  const long long bound = (long long)p.w_num * lo_lb;           // cost * w_den <= bound: within w of Lo
  int code = 0, n = 0;
  if (inc != kCbsNoKey && (long long)inc_cost * p.w_den <= bound) code = RMPC_CBS_SOLVED;
  else if (opn == kCbsNoKey) code = RMPC_CBS_INFEASIBLE;       // (no incumbent either: with one, rule 1 fired)
  else {
    // FOCAL's e least.  A pass: every thread keeps the kEcbsKeep least keys above `last` among its ids, sorted, and the
    // least key it let go; the lists' heads are merged for as long as the least head is below everything let go.
    unsigned long long last = 0;
    bool more = true;
    while (more && n < p.expand) {
      int cnt = 0;
      unsigned long long drop = kCbsNoKey;
      for (int id = tid; id < hi; id += 256) {
        if (pool.state()[id] != kCbsOpen) continue;
        const int cost = pool.cost()[id];
        if ((long long)cost * p.w_den > bound || cost >= inc_cost) continue;
        const unsigned long long key = ecbs_rank(pool.nconf()[id], cost, id);
        if (n > 0 && key <= last) continue;
        int j;
        if (cnt < kEcbsKeep) j = cnt++;
        else {
          const unsigned long long worst = lst[(kEcbsKeep - 1) * 256 + tid];
          if (key > worst) { drop = key < drop ? key : drop; continue; }
          drop = worst < drop ? worst : drop;
          j = kEcbsKeep - 1;
        }
        for (; j > 0 && lst[(j - 1) * 256 + tid] > key; j--) lst[j * 256 + tid] = lst[(j - 1) * 256 + tid];
        lst[j * 256 + tid] = key;
      }
      const unsigned long long let_go = cbs_block_min(drop, red_k, tid, 256);
      int head = 0;
      while (n < p.expand) {
        const unsigned long long mine = head < cnt ? lst[head * 256 + tid] : kCbsNoKey;
        const unsigned long long m = cbs_block_min(mine, red_k, tid, 256);
        if (m == kCbsNoKey) { more = false; break; }           // FOCAL has no more
        if (m > let_go) break;                                  // a key that was let go comes first: another pass
        if (mine == m) head++;
        if (tid == 0) takes[n] = (int)(m & 0x1fffff);
        last = m;
        n++;
      }
    }
    if (2LL * ((long long)expanded + n) >= (long long)p.nodes) code = RMPC_CBS_POOL;
  }
  __syncthreads();
  if (code) {
    if (tid == 0) { h->stop = code; h->n_take = 0; }
    return;
  }
  for (int k = tid; k < n; k += 256) {
    h->take[k] = takes[k];
    pool.state()[takes[k]] = kCbsExpanded;
  }
  if (tid == 0) { h->stop = 0; h->x0 = expanded; h->expanded = expanded + n; h->n_take = n; h->rounds_run += 1; }
}

}  // namespace rmpc
