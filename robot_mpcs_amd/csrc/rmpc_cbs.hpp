// rmpc_cbs.hpp -- optimal timed routes: conflict-based search on the device (include/rmpc_cbs.h),
// included by rmpc_world.hip behind rmpc_timed.hpp.  The rule is written out in the header; here are its three kernels.
//
//  k_cbs_root    one workgroup: the free mask, every robot's route under the empty table, node 0.
//  k_cbs_select  one workgroup, once per round and once more as the report: a pass over the ids in use finds the
//                incumbent and the least open node, decides the round (rules 1 to 3) and leaves the taken nodes in the
//                workspace's header -- or, as the report, writes the outputs.
//  k_cbs_expand  one workgroup per child, 2 E per round: the child's table from the chain of constraints, the route of
//                the constrained robot (timed_robot of rmpc_timed.hpp without a start rule and without stamping), the
//                parent's other paths, the node's conflict.
// The host enqueues root, `rounds` x (select, expand) and the report without reading anything: a kernel behind a stop
// reads the header's flag and returns.  No workgroup waits for another: what a kernel reads of other workgroups was
// written by an earlier kernel of the stream.
//
// The workspace: the header, the free mask, then per node its conflict key, parent, constraint, cost, state, the robots'
// arrive and paths as int16 (a cell is below 2^14, arrive at most 1024), then one slot per workgroup of k_cbs_expand: the
// table and the history as timed_work_at lays them out (the history in LDS up to kTimedHistLds) and the int32 path that
// timed_robot writes.

#include <climits>
#include <cstdint>

namespace rmpc {

constexpr int kCbsNone = 0, kCbsOpen = 1, kCbsSolution = 2, kCbsExpanded = 3;     // a node's state; ids not in use: none
constexpr unsigned long long kCbsNoKey = ~0ull;

struct CbsHdr {
  int magic, stop, expanded, x0, n_take, rounds_run, created, pad;
  int take[RMPC_CBS_MAX_EXPAND];
};

// byte offsets into the workspace (8-byte parts first) and the words of a slot
struct CbsLayout {
  long long freeb, conf, slots, parent, con, cost, state, arrive, paths, total;
  long long slot_words;
};

__host__ static inline CbsLayout cbs_layout(int H, int W, int T, int B, int M, int E) {
  const long long L = (long long)H * ((W + 63) / 64);
  CbsLayout y;
  y.slot_words = timed_order_words(H, W, T) + (T + 2) / 2;
  y.freeb = (long long)sizeof(CbsHdr);
  y.conf = y.freeb + 8 * L;
  y.slots = y.conf + 8LL * M;
  y.parent = y.slots + 8 * y.slot_words * 2 * E;
  y.con = y.parent + 4LL * M;
  y.cost = y.con + 4LL * M;
  y.state = y.cost + 4LL * M;
  y.arrive = y.state + 4LL * M;
  y.paths = y.arrive + 2LL * M * B;
  y.total = y.paths + 2LL * M * B * (T + 1);
  y.total = (y.total + 7) / 8 * 8;
  return y;
}

// the node arrays of a workspace, each formed from the layout where it is used: ten pointers held at once cost the root
// kernel its scalar registers
struct CbsPool {
  char *w;
  const CbsLayout &y;
  __device__ __forceinline__ CbsHdr *hdr() const { return (CbsHdr *)w; }
  __device__ __forceinline__ timed_word *freeb() const { return (timed_word *)(w + y.freeb); }
  __device__ __forceinline__ timed_word *slots() const { return (timed_word *)(w + y.slots); }
  __device__ __forceinline__ unsigned long long *conf() const { return (unsigned long long *)(w + y.conf); }
  __device__ __forceinline__ int *parent() const { return (int *)(w + y.parent); }
  __device__ __forceinline__ int *con() const { return (int *)(w + y.con); }
  __device__ __forceinline__ int *cost() const { return (int *)(w + y.cost); }
  __device__ __forceinline__ int *state() const { return (int *)(w + y.state); }
  __device__ __forceinline__ short *arrive() const { return (short *)(w + y.arrive); }
  __device__ __forceinline__ short *paths() const { return (short *)(w + y.paths); }
};

__device__ __forceinline__ CbsPool cbs_pool(void *work, const CbsLayout &y) { return {(char *)work, y}; }

// a constraint in one int32: kind (0: keep clear of v around s; 1: not on v at s), robot, layer s, cell v
__device__ __forceinline__ int cbs_con(int kind, int b, int s, int v) { return (kind << 30) | (b << 24) | (s << 14) | v; }

// no start rule: nothing is closed to a robot but its table
struct TimedNoStartRule {
  __device__ __forceinline__ void prepare(int, int) const {}
  __device__ __forceinline__ bool early(int) const { return false; }
  __device__ __forceinline__ int closed_until(int, int, timed_word) const { return -1; }
};

// the least of v over the workgroup's nt threads (a power of two); ends behind a barrier that frees red
__device__ __forceinline__ unsigned long long cbs_block_min(unsigned long long v, unsigned long long *red, int tid, int nt) {
  red[tid] = v;
  __syncthreads();
  for (int h = nt >> 1; h > 0; h >>= 1) {
    if (tid < h && red[tid + h] < red[tid]) red[tid] = red[tid + h];
    __syncthreads();
  }
  const unsigned long long r = red[0];
  __syncthreads();
  return r;
}

// the table's part of one constraint on the robot: a disc in the layers within lag of s, formed as timed_stamp forms its
// masks (one (disc row, layer) per thread and pass), or one bit
__device__ __forceinline__ void cbs_constrain(timed_word *table, int con, const TimedDims &d) {
  const int s = (con >> 14) & 1023, v = con & 16383;
  const int r0 = v / d.W, col = v - r0 * d.W;
  if (con >> 30) {
    if (d.tid == 0)
      __hip_atomic_fetch_or(table + (size_t)s * d.L + r0 * d.Wd + (col >> 6), 1ull << (col & 63), __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const int side = 2 * d.rad + 1, nl = 2 * d.lag + 1;
  for (int i = d.tid; i < side * nl; i += d.nt) {
    const int dr = i / nl - d.rad, u = s - d.lag + (i - (i / nl) * nl), r = r0 + dr;
    if (u < 1 || u > d.T || r < 0 || r >= d.H) continue;
    const int h = timed_half_width(dr, d.rad, d.sep2);
    const int lo = col - h > 0 ? col - h : 0, hi = col + h < d.W - 1 ? col + h : d.W - 1;
    for (int j = lo >> 6; j <= hi >> 6; j++) {
      const int a = (lo > j * 64 ? lo : j * 64) - j * 64, e = (hi < j * 64 + 63 ? hi : j * 64 + 63) - j * 64;
      const timed_word mask = (e == 63 ? ~0ull : (1ull << (e + 1)) - 1ull) & ~((1ull << a) - 1ull);
      __hip_atomic_fetch_or(table + (size_t)u * d.L + r * d.Wd + j, mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// the node's conflict as the key (min(t, s) << 32) | (i << 26) | (j << 20) | (t << 10) | s, kCbsNoKey without one: robot
// i by robot i, the threads stride over (j > i, t) and each looks at the layers s within lag of t.  paths was written
// by this workgroup behind a barrier; ends behind a barrier.
__device__ __forceinline__ unsigned long long cbs_conflict(const short *paths, int B, int T, int W, int sep2, int lag,
                                                           unsigned long long *red, int tid, int nt) {
  unsigned long long best = kCbsNoKey;
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
        }
      }
    }
  }
  return cbs_block_min(best, red, tid, nt);
}

// what the root and the children share: the dims, the slot of this workgroup and the route of robot b under the table
// that the slot holds; true when the route exists.  path32: the slot's int32 path; *arrive: thread 0's.
template <bool kLds>
__device__ __forceinline__ TimedWork cbs_slot(const CbsPool &pool, const CbsLayout &y, int slot, const TimedGeom &q, int T) {
  TimedWork wk = timed_work_at<kLds>(pool.slots(), slot, q, T);
  wk.freeb = pool.freeb();                                       // the one free mask, made by the root
  return wk;
}

__device__ __forceinline__ void cbs_clear_table(const TimedWork &wk, const TimedDims &d) {
  for (size_t i = d.tid; i < (size_t)(d.T + 1) * d.L; i += d.nt)
    __hip_atomic_store(wk.res + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool cbs_skipped(const rmpc_cbs &p, int b) {
  const int s = p.start_cell[b], gi = p.goal_index[b];
  return s < 0 || s >= p.H * p.W || gi < 0 || gi >= p.Gf;
}

template <bool kLds>
__global__ __launch_bounds__(kTimedThreads) void k_cbs_root(rmpc_cbs p, TimedGeom q, CbsLayout y, int magic) {
  __shared__ unsigned long long red_k[kTimedThreads];
  __shared__ int red_c[kTimedThreads];
  __shared__ int sa[2];
  const int tid = threadIdx.x, nt = blockDim.x, B = p.B, T = p.T;
  const TimedDims d = {p.H, p.W, q.Wd, q.L, T, p.lag, p.sep2, q.rad, p.movement, tid, nt};
  const CbsPool pool = cbs_pool(p.work, y);
  const TimedWork wk = cbs_slot<kLds>(pool, y, 0, q, T);
  int *const path32 = (int *)(wk.res + (q.per_order - (T + 2) / 2));       // behind the planner's parts
  timed_free_mask(pool.freeb(), p.grid, p.occ_threshold, d);
  cbs_clear_table(wk, d);
  __syncthreads();
  TimedNoStartRule rule;
  bool dead = false;
  int cost = 0;                                                // thread 0's
  for (int b = 0; b < B; b++) {
    short *const path = pool.paths() + (size_t)b * (T + 1);
    if (cbs_skipped(p, b)) {
      for (int t = tid; t <= T; t += nt) path[t] = -1;
      if (tid == 0) { pool.arrive()[b] = (short)(T + 1); cost += T + 1; }
      continue;
    }
    const TimedEnd e = timed_robot<false, false>(d, wk, rule, p.fields, p.goal_cells, p.start_cell[b], 0, 0, nullptr,
                                                 p.goal_index[b], 0, path32, nullptr, sa, sa + 1, (double *)red_k, red_c);
    if (e.f) { dead = true; break; }                           // (uniform)
    for (int t = tid; t <= T; t += nt) path[t] = (short)path32[t];
    if (tid == 0) { pool.arrive()[b] = (short)e.a; cost += e.a; }
    __syncthreads();                                           // path32 is read before the next robot writes it
  }
  unsigned long long key = kCbsNoKey;
  if (!dead) {
    __syncthreads();
    key = cbs_conflict(pool.paths(), B, T, p.W, p.sep2, p.lag, red_k, tid, nt);
  }
  if (tid == 0) {
    CbsHdr *const h = pool.hdr();
    h->magic = magic; h->stop = 0; h->expanded = 0; h->x0 = 0; h->n_take = 0; h->rounds_run = 0; h->created = dead ? 0 : 1;
    pool.parent()[0] = -1; pool.con()[0] = 0; pool.cost()[0] = cost; pool.conf()[0] = key;
    pool.state()[0] = dead ? kCbsNone : (key == kCbsNoKey ? kCbsSolution : kCbsOpen);
  }
}

template <bool kLds>
__global__ __launch_bounds__(kTimedThreads) void k_cbs_expand(rmpc_cbs p, TimedGeom q, CbsLayout y) {
  __shared__ unsigned long long red_k[kTimedThreads];
  __shared__ int red_c[kTimedThreads];
  __shared__ int sa[2];
  const int tid = threadIdx.x, nt = blockDim.x, B = p.B, T = p.T, T1 = T + 1;
  const CbsPool pool = cbs_pool(p.work, y);
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
  const TimedWork wk = cbs_slot<kLds>(pool, y, blockIdx.x, q, T);
  int *const path32 = (int *)(wk.res + (q.per_order - (T + 2) / 2));       // behind the planner's parts
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
                                               p.goal_index[r], 0, path32, nullptr, sa, sa + 1, (double *)red_k, red_c);
  if (e.f) {                                                   // the route does not exist: the child is dead
    if (tid == 0) pool.state()[id] = kCbsNone;
    return;
  }
  short *const paths = pool.paths() + (size_t)id * B * T1;
  for (int i = tid; i < B * T1; i += nt) {
    const int b = i / T1;
    paths[i] = b == r ? (short)path32[i - b * T1] : ppaths[i];
  }
  for (int b = tid; b < B; b += nt) pool.arrive()[(size_t)id * B + b] = b == r ? (short)sa[1] : pool.arrive()[(size_t)parent * B + b];
  __syncthreads();
  const unsigned long long key = cbs_conflict(paths, B, T, p.W, p.sep2, p.lag, red_k, tid, nt);
  if (tid == 0) {
    pool.parent()[id] = parent; pool.con()[id] = con; pool.conf()[id] = key;
    pool.cost()[id] = pool.cost()[parent] - (int)pool.arrive()[(size_t)parent * B + r] + e.a;
    pool.state()[id] = key == kCbsNoKey ? kCbsSolution : kCbsOpen;
    atomicAdd(&pool.hdr()->created, 1);
  }
}

// One round's decision, or with `report` the outputs.  `first`: the first kernel of a call that reads the header -- it
// checks that the workspace holds a search of these arguments and takes no earlier stop for its own.
__global__ __launch_bounds__(256) void k_cbs_select(rmpc_cbs p, CbsLayout y, int magic, int first, int report) {
  __shared__ unsigned long long red_k[256];
  __shared__ int takes[RMPC_CBS_MAX_EXPAND];
  const int tid = threadIdx.x, B = p.B, T = p.T, T1 = T + 1;
  const CbsPool pool = cbs_pool(p.work, y);
  CbsHdr *const h = pool.hdr();
  const bool bad = h->magic != magic;
  const int stop = first ? (bad ? RMPC_CBS_BAD_STATE : 0) : h->stop;
  __syncthreads();                                             // every thread has read the flag before thread 0 sets it
  if (stop != 0 && !report) {
    if (first && tid == 0) { h->stop = stop; h->n_take = 0; }
    return;
  }
  unsigned long long inc = kCbsNoKey, lo = kCbsNoKey;
  const int expanded = bad ? 0 : h->expanded;
  if (!bad) {
    const int hi = 1 + 2 * expanded;
    unsigned long long mi = kCbsNoKey, ml = kCbsNoKey;
    for (int id = tid; id < hi; id += 256) {
      const int st = pool.state()[id];
      const unsigned long long key = ((unsigned long long)(unsigned)pool.cost()[id] << 32) | (unsigned)id;
      if (st == kCbsOpen) ml = key < ml ? key : ml;
      else if (st == kCbsSolution) mi = key < mi ? key : mi;
    }
    inc = cbs_block_min(mi, red_k, tid, 256);
    lo = cbs_block_min(ml, red_k, tid, 256);
  }
  const int inc_cost = inc == kCbsNoKey ? RMPC_CBS_INF : (int)(inc >> 32);
  const int lo_cost = lo == kCbsNoKey ? RMPC_CBS_INF : (int)(lo >> 32);

  if (report) {
    const unsigned long long best = inc != kCbsNoKey ? inc : lo;
    const int node = best == kCbsNoKey ? -1 : (int)(unsigned)best;
    if (tid == 0) {
      if (first) h->stop = stop;
      int *const o = p.info;
      o[RMPC_CBS_OUTCOME] = stop ? stop : RMPC_CBS_ROUNDS;
      o[RMPC_CBS_NODE] = node;
      o[RMPC_CBS_CONFLICT_FREE] = inc != kCbsNoKey;
      o[RMPC_CBS_COST] = node < 0 ? RMPC_CBS_INF : (int)(best >> 32);
      o[RMPC_CBS_BOUND] = lo_cost < inc_cost ? lo_cost : inc_cost;
      o[RMPC_CBS_CREATED] = bad ? 0 : h->created;
      o[RMPC_CBS_EXPANDED] = expanded;
      o[RMPC_CBS_ROUNDS_RUN] = bad ? 0 : h->rounds_run;
    }
    for (int i = tid; i < B * T1; i += 256) p.paths[i] = node < 0 ? -1 : (int)pool.paths()[(size_t)node * B * T1 + i];
    for (int b = tid; b < B; b += 256) {
      p.arrive[b] = node < 0 ? T + 1 : (int)pool.arrive()[(size_t)node * B + b];
      p.status[b] = cbs_skipped(p, b) ? RMPC_GRID_OUTSIDE : 0;
    }
    return;
  }

  int code = 0, n = 0;
  if (inc != kCbsNoKey && inc_cost <= lo_cost) code = RMPC_CBS_SOLVED;
  else if (lo == kCbsNoKey) code = RMPC_CBS_INFEASIBLE;
  else {
    // the least open node is takeable (its cost is below the incumbent's); then the next ones above it, one pass each
    const int hi = 1 + 2 * expanded;
    unsigned long long last = lo;
    if (tid == 0) takes[0] = (int)(unsigned)lo;
    for (n = 1; n < p.expand; n++) {
      unsigned long long m = kCbsNoKey;
      for (int id = tid; id < hi; id += 256) {
        const unsigned long long key = ((unsigned long long)(unsigned)pool.cost()[id] << 32) | (unsigned)id;
        if (pool.state()[id] == kCbsOpen && key > last && pool.cost()[id] < inc_cost) m = key < m ? key : m;
      }
      m = cbs_block_min(m, red_k, tid, 256);
      if (m == kCbsNoKey) break;
      if (tid == 0) takes[n] = (int)(unsigned)m;
      last = m;
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
