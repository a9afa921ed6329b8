// rmpc_tours.hpp -- tours of several tasks per robot on the device and the follower that stops at them
// (include/rmpc_tours.h), included by rmpc_world.hip behind rmpc_assign_opt.hpp, whose wave reductions it
// uses.  Three kernels: k_tours_quantise turns the fp64 costs of all problems into the int32 matrices of the workspace
// over the whole chip, k_tours runs the build and the improvement of the header, one workgroup per problem, and
// k_follow_tour is k_follow_path with stops.  Every choice is a minimum of integers under a strict total order, so no
// result depends on the order in which lanes meet.  Contraction is off, as in rmpc_assign_opt.hpp.

namespace rmpc {

constexpr int kToursMaxRobots = RMPC_TOURS_MAX_ROBOTS, kToursMaxTasks = RMPC_TOURS_MAX_TASKS;
// the index part of a key: (b, t, k) of a build candidate, (kind, i, j, l) of a move
constexpr int kToursHiShift = 21, kToursMidShift = 11, kToursKindShift = 31;
constexpr unsigned long long kToursNone = ~0ull;
// the leading part, biased to be non-negative: |delta| <= 3 * 2^20, |ds| <= 6 * 2^20, |pm_new - pm_old| <= 2^30
constexpr long long kToursDeltaBias = 1ll << 23, kToursDsBias = 1ll << 24, kToursPmBias = 1ll << 31;
constexpr int kToursDsBits = 25;
static_assert(kToursMaxRobots <= 1024 && kToursMaxTasks <= 1024 && (long long)kToursMaxTasks * kAssignOptMaxQ <= (1ll << 30) &&
              6ll * kAssignOptMaxQ < kToursDeltaBias,
              "k_tours: a robot, a task and a position (<= 1024) in 10, 10 and 11 bits; a tour's cost in an int32");

// "no insertion" in the table of cheapest insertions (an insertion's cost lies within 3 * 2^20 of 0)
constexpr int kToursNoIns = INT_MIN;

// the workspace, int32 each: qs [G][B][T], qt [G][T][T] and its transpose qtT [G][T][T], then per (robot, task) the
// cheapest insertion of the task into the robot's tour as it stands and its position, ins [G][B][T] and pos [G][B][T]
__host__ __device__ inline long long tours_work_ints(int G, int B, int T) {
  return 3ll * G * B * T + 2ll * G * T * T;
}

// One lane per entry of the start costs (the first nstart = G B T lanes) and of the task costs (G T T more): q of the
// edge, or -1 when it is not takeable.  A task cost is written twice, to qt [g][i][j] and to qtT [g][j][i], so that a lane
// which owns a task t finds both D [x][t] and D [t][x] next to its neighbours'.  Into an empty tour a task goes at
// position 0 for the start's edge: that is the first state of the table of cheapest insertions.
__global__ __launch_bounds__(256) void k_tours_quantise(int T, long long nstart, long long total,
                                                        const double *__restrict__ start_cost,
                                                        const double *__restrict__ task_cost, double scale,
                                                        int *__restrict__ qs, int *__restrict__ qt, int *__restrict__ qtT,
                                                        int *__restrict__ ins, int *__restrict__ pos) {
#pragma clang fp contract(off)
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const bool start = idx < nstart;
  const long long e = start ? idx : idx - nstart;
  const double c = start ? start_cost[e] : task_cost[e];
  const double r = __builtin_rint(c * scale);
  const int q = c >= 0.0 && c < __builtin_inf() && r <= (double)kAssignOptMaxQ ? (int)r : -1;
  if (start) { qs[e] = q; ins[e] = q < 0 ? kToursNoIns : q; pos[e] = 0; return; }
  const int TT = T * T;                                      // G T T <= INT_MAX
  const int g = (int)(e / TT), rem = (int)(e - (long long)g * TT), i = rem / T, j = rem - i * T;
  qt[e] = q;
  qtT[(long long)g * TT + (long long)j * T + i] = q;
}

// The tours of one problem in LDS: linked lists over the tasks.  next / prev: the neighbours of an assigned task in its
// tour (-1: none; the predecessor of a first task is its robot's start), owner: its robot (-1: unassigned), ein: the q
// of the edge into it; head, len, c per robot, c [b] the sum of ein along the tour (at most 2^30).
struct ToursState {
  int *next, *prev, *owner, *ein, *head, *len, *c;
  const int *qs, *qt;
  int T;
  // q of the edge from `pred` (a task, or the start of b when -1) to the task t
  __device__ __forceinline__ int edge(int b, int pred, int t) const { return pred < 0 ? qs[b * T + t] : qt[pred * T + t]; }
  // t, unassigned, goes to position k of tour b; both new edges are takeable
  __device__ void insert(int b, int t, int k) const {
    int pred = -1, succ = head[b];
    for (int i = 0; i < k; i++) { pred = succ; succ = next[succ]; }
    const int first = edge(b, pred, t);
    int cb = c[b] + first;
    owner[t] = b; prev[t] = pred; next[t] = succ; ein[t] = first;
    if (pred < 0) head[b] = t; else next[pred] = t;
    if (succ >= 0) {
      const int second = qt[t * T + succ];
      prev[succ] = t;
      cb += second - ein[succ];
      ein[succ] = second;
    }
    c[b] = cb;
    len[b]++;
  }
  // t leaves its tour; the bridging edge is takeable
  __device__ void remove(int t) const {
    const int b = owner[t], pred = prev[t], succ = next[t];
    int cb = c[b] - ein[t];
    if (pred < 0) head[b] = succ; else next[pred] = succ;
    if (succ >= 0) {
      const int bridge = edge(b, pred, succ);
      prev[succ] = pred;
      cb += bridge - ein[succ];
      ein[succ] = bridge;
    }
    c[b] = cb;
    len[b]--;
    owner[t] = -1;
    ein[t] = 0;
  }
  // x stands directly in front of y: pred, x, y, succ becomes pred, y, x, succ
  __device__ void swap_adjacent(int x, int y) const {
    const int b = owner[x], pred = prev[x], succ = next[y];
    const int ey = edge(b, pred, y), ex = qt[y * T + x];
    int cb = c[b] + (ey - ein[x]) + (ex - ein[y]);
    if (pred < 0) head[b] = y; else next[pred] = y;
    prev[y] = pred; next[y] = x; prev[x] = y; next[x] = succ;
    ein[y] = ey; ein[x] = ex;
    if (succ >= 0) {
      const int es = qt[x * T + succ];
      prev[succ] = x;
      cb += es - ein[succ];
      ein[succ] = es;
    }
    c[b] = cb;
  }
  // two assigned tasks change places
  __device__ void exchange(int a, int b) const {
    const int na = next[a], nb = next[b];
    if (na == b) { swap_adjacent(a, b); return; }
    if (nb == a) { swap_adjacent(b, a); return; }
    const int ra = owner[a], rb = owner[b], pa = prev[a], pb = prev[b];
    const int eb = edge(ra, pa, b), ea = edge(rb, pb, a);    // b in a's place, a in b's
    const int old_a = ein[a], old_b = ein[b];
    owner[a] = rb; owner[b] = ra;
    prev[b] = pa; next[b] = na; prev[a] = pb; next[a] = nb;
    if (pa < 0) head[ra] = b; else next[pa] = b;
    if (pb < 0) head[rb] = a; else next[pb] = a;
    ein[b] = eb; ein[a] = ea;
    int da = eb - old_a, db = ea - old_b;
    if (na >= 0) { const int e = qt[b * T + na]; prev[na] = b; da += e - ein[na]; ein[na] = e; }
    if (nb >= 0) { const int e = qt[a * T + nb]; prev[nb] = a; db += e - ein[nb]; ein[nb] = e; }
    c[ra] += da;
    c[rb] += db;                                             // (one thread: ra == rb adds both)
  }
};

// The build and the improvement of include/rmpc_tours.h for problem blockIdx.x, with blockDim.x = T rounded up to whole
// wavefronts, at most MAXT.  Thread t owns task t.
//
// A step changes one or two tours, so the cheapest insertion of a task into a tour it is not in -- the least
// (ins, position) over the tour's positions -- is kept per (robot, task) in the workspace, ins [b][t] and pos [b][t],
// column t read and written by thread t alone.  refresh(b) walks the positions of tour b -- the walk is the same in all
// lanes, so the predecessor and the successor are wave-uniform and D [pred][t], D [t][succ] (from the transpose) are read
// from consecutive addresses across the lanes -- and is called for the tours the last step changed.  Among the
// positions of one tour the one of least ins, the first of equals, is also the least in every order of the header:
// c [b] + ins, ds = ins - rem and pm_new = max(c1 - rem, c2 + ins) rise with ins, and the position comes last.
//
// A build step: a thread whose task is unassigned reads its row of the table, one entry per tour that has room, from
// consecutive addresses across the lanes, and keeps its least (lead, index).  The workgroup takes the least of those:
// the least lead by a DPP reduction inside each wave, then the least index among the lanes that hold it, then the
// waves' pairs through LDS slots that alternate between steps.  The thread of the winning task inserts it, a second
// barrier ends the step, and every thread refreshes its entry of the tour that grew.
//
// An improvement round: a thread whose task t is assigned reads the table for the relocations of t into the other
// tours, walks its own tour without t for those within it, then the tasks u > t for the exchanges (t, u); the
// reduction is the same, the thread of the move's first task applies it and names the touched tours in LDS.
//
// Every loop is bounded by a counter: the build by T steps, a walk by the tour's length, the rounds by max_rounds.
template <int MAXT>
__global__ __launch_bounds__(MAXT) void k_tours(int B, int T, int K, int mode, int max_rounds,
                                                const int *__restrict__ qs_all, const int *__restrict__ qt_all,
                                                const int *__restrict__ qtT_all, int *ins_all, int *pos_all,
                                                int *__restrict__ tours_out,
                                                int *__restrict__ len_out, long long *__restrict__ cost_out,
                                                int *__restrict__ owner_out, int *__restrict__ count_out,
                                                long long *__restrict__ total_out, long long *__restrict__ span_out,
                                                int *__restrict__ build_out, int *__restrict__ rounds_out) {
  static_assert(MAXT % 64 == 0 && MAXT <= 1024, "k_tours: whole wavefronts");
  __shared__ int s_next[MAXT], s_prev[MAXT], s_owner[MAXT], s_ein[MAXT];
  __shared__ int s_head[kToursMaxRobots], s_len[kToursMaxRobots], s_c[kToursMaxRobots];
  __shared__ unsigned long long s_key[2][MAXT / 64][2];
  __shared__ int s_touched[2];
  const int g = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, nw = nt >> 6;
  const int *const qs = qs_all + (size_t)g * B * T, *const qt = qt_all + (size_t)g * T * T,
            *const qtT = qtT_all + (size_t)g * T * T;
  int *const c_ins = ins_all + (size_t)g * B * T, *const c_pos = pos_all + (size_t)g * B * T;
  const ToursState S{s_next, s_prev, s_owner, s_ein, s_head, s_len, s_c, qs, qt, T};
  const int t = tid;
  const bool mine = t < T;
  if (mine) { s_next[t] = -1; s_prev[t] = -1; s_owner[t] = -1; s_ein[t] = 0; }
  for (int b = tid; b < B; b += nt) { s_head[b] = -1; s_len[b] = 0; s_c[b] = 0; }
  __syncthreads();
  int par = 0;
  // the least (hi, lo) of the workgroup in every thread; all threads call it
  auto least = [&](unsigned long long &hi, unsigned long long &lo) {
    const unsigned long long m = assign_opt_wave_min(hi);
    lo = assign_opt_wave_min(hi == m ? lo : kToursNone);
    hi = m;
    if constexpr (MAXT > 64) {
      if ((tid & 63) == 0) { s_key[par][tid >> 6][0] = hi; s_key[par][tid >> 6][1] = lo; }
      __syncthreads();
      for (int w = 0; w < nw; w++) {
        const unsigned long long oh = s_key[par][w][0], ol = s_key[par][w][1];
        if (oh < hi || (oh == hi && ol < lo)) { hi = oh; lo = ol; }
      }
      par ^= 1;
    }
  };

  // the thread's entry of tour b: the least (ins, position) of its task over the tour as it stands; a task of the tour
  // itself has no entry (it is never read)
  auto refresh = [&](int b) {
    if (!mine || s_owner[t] == b) return;
    const int n = s_len[b];
    int best = kToursNoIns, at = 0, pred = -1, succ = s_head[b];
    for (int k = 0; k <= n; k++) {
      const int first = pred < 0 ? qs[b * T + t] : qt[pred * T + t];
      int second = 0, old = 0;
      if (succ >= 0) { second = qtT[succ * T + t]; old = s_ein[succ]; }
      if (first >= 0 && second >= 0) {
        const int ins = first + second - old;
        if (best == kToursNoIns || ins < best) { best = ins; at = k; }   // k ascends: the first of equals stays
      }
      pred = succ;
      if (succ >= 0) succ = s_next[succ];
    }
    c_ins[b * T + t] = best;
    c_pos[b * T + t] = at;
  };

  int build_steps = 0;
  for (; build_steps < T; build_steps++) {
    unsigned long long hi = kToursNone, lo = kToursNone;
    if (mine && s_owner[t] < 0) {
      for (int b = 0; b < B; b++) {
        if (s_len[b] >= K) continue;
        const int ins = c_ins[b * T + t];
        if (ins == kToursNoIns) continue;
        const unsigned long long lead = (unsigned long long)(mode ? (long long)s_c[b] + ins : ins + kToursDeltaBias);
        if (lead < hi) {                                     // b ascends within a thread: the first of equals stays
          hi = lead;
          lo = ((unsigned long long)b << kToursHiShift) | ((unsigned)t << kToursMidShift) | (unsigned)c_pos[b * T + t];
        }
      }
    }
    least(hi, lo);
    if (hi == kToursNone) break;
    const int wt = (int)(lo >> kToursMidShift) & 1023, wb = (int)(lo >> kToursHiShift);
    if (tid == wt) S.insert(wb, wt, (int)lo & 2047);
    __syncthreads();
    refresh(wb);
  }

  int rounds = 0;
  for (; rounds < max_rounds; rounds++) {
    unsigned long long hi = kToursNone, lo = kToursNone;
    // (lead, index) of an admissible move against the thread's least; the index ascends within a thread
    auto offer = [&](long long ds, long long pm_old, long long pm_new, unsigned long long index) {
      const long long pmd = pm_new - pm_old;
      if (mode ? !(pmd < 0 || (pmd == 0 && ds < 0)) : !(ds < 0)) return;
      const unsigned long long lead =
          mode ? ((unsigned long long)(pmd + kToursPmBias) << kToursDsBits) | (unsigned long long)(ds + kToursDsBias)
               : (unsigned long long)(ds + kToursDsBias);
      if (lead < hi) { hi = lead; lo = index; }
    };
    if (mine && s_owner[t] >= 0) {
      const int b1 = s_owner[t], p = s_prev[t], n = s_next[t], ein_t = s_ein[t];
      const int eout_t = n >= 0 ? s_ein[n] : 0;
      const long long c1 = s_c[b1];
      const int bridge = n >= 0 ? S.edge(b1, p, n) : 0;
      if (bridge >= 0) {
        const long long rem = (long long)ein_t + eout_t - bridge;
        for (int b2 = 0; b2 < B; b2++) {
          const unsigned long long index = ((unsigned long long)t << kToursHiShift) | ((unsigned)b2 << kToursMidShift);
          if (b2 != b1) {                                    // into another tour: the table's entry
            if (s_len[b2] >= K) continue;
            const int entry = c_ins[b2 * T + t];
            if (entry == kToursNoIns) continue;
            const long long ins = entry, c2 = s_c[b2];
            offer(ins - rem, c1 > c2 ? c1 : c2, c1 - rem > c2 + ins ? c1 - rem : c2 + ins, index | (unsigned)c_pos[b2 * T + t]);
            continue;
          }
          const int len1 = s_len[b1];                        // within its own tour: the positions of the tour without t
          int pred = -1, succ = s_head[b1], shift = 0;
          for (int k = 0; k <= len1; k++) {
            if (succ == t || pred == t) {                    // the two gaps beside t: together the no-op
              if (pred == t) shift = 1;
            } else {
              const int first = pred < 0 ? qs[b1 * T + t] : qt[pred * T + t];
              int second = 0, old = 0;
              if (succ >= 0) { second = qtT[succ * T + t]; old = s_ein[succ]; }
              if (first >= 0 && second >= 0) {
                const long long ds = (long long)first + second - old - rem;
                offer(ds, c1, c1 + ds, index | (unsigned)(k - shift));
              }
            }
            pred = succ;
            if (succ >= 0) succ = s_next[succ];
          }
        }
      }
      for (int u = t + 1; u < T; u++) {
        const int b2 = s_owner[u];
        if (b2 < 0) continue;
        const int pu = s_prev[u], nu = s_next[u], ein_u = s_ein[u];
        const int eout_u = nu >= 0 ? s_ein[nu] : 0;
        const unsigned long long index = (1ull << kToursKindShift) | ((unsigned long long)t << kToursHiShift) |
                                         ((unsigned)u << kToursMidShift);
        if (n == u) {                                        // p, t, u, nu -> p, u, t, nu
          const int e1 = S.edge(b1, p, u), mid = qt[u * T + t], e4 = nu >= 0 ? qt[t * T + nu] : 0;
          if (e1 >= 0 && mid >= 0 && e4 >= 0) {
            const long long ds = (long long)e1 + mid + e4 - ((long long)ein_t + ein_u + eout_u);
            offer(ds, c1, c1 + ds, index);
          }
        } else if (nu == t) {                                // pu, u, t, n -> pu, t, u, n
          const int e3 = S.edge(b2, pu, t), mid = qt[t * T + u], e2 = n >= 0 ? qt[u * T + n] : 0;
          if (e3 >= 0 && mid >= 0 && e2 >= 0) {
            const long long ds = (long long)e3 + mid + e2 - ((long long)ein_u + ein_t + eout_t);
            offer(ds, c1, c1 + ds, index);
          }
        } else {
          // (D [p][u] and D [t][nu] from the transpose: row u, and consecutive addresses across the lanes)
          const int e1 = p < 0 ? qs[b1 * T + u] : qtT[u * T + p], e2 = n >= 0 ? qt[u * T + n] : 0;
          const int e3 = S.edge(b2, pu, t), e4 = nu >= 0 ? qtT[nu * T + t] : 0;
          if (e1 >= 0 && e2 >= 0 && e3 >= 0 && e4 >= 0) {
            const long long da = (long long)e1 + e2 - ein_t - eout_t, db = (long long)e3 + e4 - ein_u - eout_u, ds = da + db;
            const long long c2 = s_c[b2];
            if (b2 == b1) offer(ds, c1, c1 + ds, index);
            else offer(ds, c1 > c2 ? c1 : c2, c1 + da > c2 + db ? c1 + da : c2 + db, index);
          }
        }
      }
    }
    least(hi, lo);
    if (hi == kToursNone) break;
    const int i = (int)(lo >> kToursHiShift) & 1023, j = (int)(lo >> kToursMidShift) & 1023;
    if (tid == i) {
      s_touched[0] = s_owner[i];
      if ((lo >> kToursKindShift) & 1) { s_touched[1] = s_owner[j]; S.exchange(i, j); }
      else { s_touched[1] = j; S.remove(i); S.insert(j, i, (int)lo & 2047); }
    }
    __syncthreads();
    const int b0 = s_touched[0], b1 = s_touched[1];
    refresh(b0);
    if (b1 != b0) refresh(b1);
  }

  // the report
  for (int b = tid; b < B; b += nt) {
    int *const row = tours_out + ((size_t)g * B + b) * K;
    const int n = s_len[b];
    int u = s_head[b];
    for (int k = 0; k < K; k++) {
      row[k] = k < n ? u : -1;
      if (k < n) u = s_next[u];
    }
    len_out[(size_t)g * B + b] = n;
    cost_out[(size_t)g * B + b] = s_c[b];
  }
  if (owner_out && mine) owner_out[(size_t)g * T + t] = s_owner[t];
  if (tid == 0) {
    long long total = 0, span = 0;
    int count = 0;
    for (int b = 0; b < B; b++) {
      const long long cb = s_c[b];
      total += cb;
      span = cb > span ? cb : span;
      count += s_len[b];
    }
    if (count_out) count_out[g] = count;
    if (total_out) total_out[g] = total;
    if (span_out) span_out[g] = span;
    if (build_out) build_out[g] = build_steps;
    if (rounds_out) rounds_out[g] = rounds;
  }
}

// k_follow_path with stops (the rule stands in include/rmpc_tours.h): one thread per robot
__global__ __launch_bounds__(256) void k_follow_tour(const int *__restrict__ path, const int *__restrict__ len, int max_len,
                                                     int *__restrict__ idx, const double *__restrict__ pos, int stride, int B,
                                                     int W, double x0, double y0, double cell, double threshold,
                                                     double *__restrict__ goal, int K, const int *__restrict__ stop_at,
                                                     int *__restrict__ leg, int *__restrict__ served, int now, double stop_tol) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int L = len[b];
  if (L <= 0) return;
  const int *const p = path + (size_t)b * max_len, *const stops = stop_at + (size_t)b * K;
  int i = idx[b], lg = leg[b];
  i = i < 0 ? 0 : (i >= L ? L - 1 : i);
  lg = lg < 0 ? 0 : lg;
  int c = p[i];
  const double dx = x0 + (double)(c % W) * cell - pos[(size_t)b * stride];
  const double dy = y0 + (double)(c / W) * cell - pos[(size_t)b * stride + 1];
  const double dist = sqrt(dx * dx + dy * dy);
  if (lg < K && stops[lg] == i) {
    if (dist <= stop_tol) {
      served[(size_t)b * K + lg] = now;
      lg++;
      if (i < L - 1 && !(lg < K && stops[lg] == i)) i++;
    }
  } else if (i < L - 1 && dist <= threshold) {
    i++;
  }
  c = p[i];
  idx[b] = i;
  leg[b] = lg;
  goal[(size_t)b * 3] = x0 + (double)(c % W) * cell;
  goal[(size_t)b * 3 + 1] = y0 + (double)(c / W) * cell;
  goal[(size_t)b * 3 + 2] = 0.0;
}

}  // namespace rmpc
