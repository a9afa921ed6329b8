// rmpc_timed_repair.hpp -- timed routes whose failing priority orders are repaired on the device
// (include/rmpc_timed_repair.h), included by rmpc_world.hip behind rmpc_timed.hpp: k_timed_plan_repair is
// k_timed_plan inside a loop over rounds.  A round plans the order it is handed with the parts of rmpc_timed.hpp as they
// stand (timed_robot under the later-starts rule, TimedKey); what is new is between two rounds: who was bad, the stable
// partition that puts the bad robots in front, whether that changed the order, and which round's plan the row reports.
//
// Round 0 plans straight into the outputs (it is the best so far by definition); every later round plans into the row's
// slot of the workspace, and the whole workgroup copies the slot to the outputs only when (key, round) improves.
//
// The partition of B <= 1024 ranks: rank k belongs to segment k / 64, which is one wave's 64 lanes in one pass of the
// workgroup over the ranks (the block is a multiple of 64 threads).  A wave ballots "bad" for its segment and leaves the
// 64-bit mask in LDS; behind one barrier every thread knows every segment's mask, and a rank's new place is a popcount
// of the masks below it: bad ranks before it (for a bad one), or all bad ranks plus the good ones before it.

#include <climits>
#include <cstdint>

namespace rmpc {

constexpr int kTimedSegments = RMPC_TIMED_MAX_ROBOTS / 64;

// what the repair adds to rmpc_timed_plan
struct TimedRepair {
  int rounds;
  int *order_out, *rounds_run, *round_best;    // [G][B], [G], [G]
};

// words of workspace of one row behind the G orders' parts: the slot (paths, status, arrive) and two orders, as int32
__host__ __device__ static inline long long timed_repair_words(int T, int B) { return ((long long)B * (T + 1) + 4LL * B + 1) / 2; }

// rule 3 of the repair: failed, or planned and not at its goal by T; a skipped robot (status < 0) is neither
__device__ __forceinline__ bool timed_repair_bad(int status, int arrive, int T) {
  return status > 0 || (status == 0 && arrive > T);
}

// next = the bad ranks of cur in their order, then the others in theirs; returns the number of bad ranks, `changed`
// whether next differs from cur.  Called by the whole workgroup under uniform control flow, behind a barrier that made
// status and arrive visible; ends behind a barrier.  seg: kTimedSegments words of LDS.
__device__ __forceinline__ int timed_repair_partition(const int *cur, int *next, const int *status, const int *arrive, int B,
                                                      int T, int tid, int nt, timed_word *seg, bool &changed) {
  const int lane = tid & 63;
  for (int k0 = 0; k0 < B; k0 += nt) {               // (the trip count is the workgroup's: every lane ballots)
    const int k = k0 + tid;
    bool bad = false;
    if (k < B) {
      const int b = cur[k];
      bad = timed_repair_bad(status[b], arrive[b], T);
    }
    const timed_word m = __ballot(bad);
    if (lane == 0) seg[k >> 6] = m;                  // k < ceil(B / nt) nt <= 1024: nt divides 1024
  }
  __syncthreads();
  const int nseg = (B + 63) >> 6;
  int nbad = 0;
  for (int s = 0; s < nseg; s++) nbad += __popcll(seg[s]);
  bool moved = false;
  for (int k0 = 0; k0 < B; k0 += nt) {
    const int k = k0 + tid;
    if (k < B) {
      const int s = k >> 6;
      int before = 0;                                // bad ranks in the segments below
      for (int j = 0; j < s; j++) before += __popcll(seg[j]);
      const timed_word m = seg[s];
      const int below = __popcll(m & ((1ull << lane) - 1ull));
      const int pos = (m >> lane) & 1ull ? before + below : nbad + (s * 64 - before) + (lane - below);
      next[pos] = cur[k];
      moved = moved || pos != k;
    }
  }
  changed = __syncthreads_or(moved);
  return nbad;
}

// One workgroup per priority order, as k_timed_plan, round after round.  Every exit of the round loop is decided on
// values that are the same in every thread: the round number, a key read from LDS behind a barrier, the ballots' sum and
// a __syncthreads_or.
template <bool kLds>
__global__ __launch_bounds__(kTimedThreads) void k_timed_plan_repair(rmpc_timed_plan p, TimedRepair x, TimedGeom q,
                                                                     timed_word *__restrict__ work) {
  __shared__ double red_d[kTimedThreads];
  __shared__ int red_c[kTimedThreads];
  __shared__ timed_word seg[kTimedSegments];
  __shared__ long long round_key;
  const int g = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, B = p.B, T = p.T, HW = p.H * p.W;
  const TimedDims d = {p.H, p.W, q.Wd, q.L, T, p.lag, p.sep2, q.rad, p.movement, tid, nt};
  const int *const row = p.orders + (size_t)g * B;
  int *const order_out = x.order_out + (size_t)g * B;
  const TimedOut out = {p.status + (size_t)g * B, p.arrive + (size_t)g * B, p.paths + (size_t)g * B * (T + 1), p.key + g,
                        nullptr, nullptr, nullptr};
  if (timed_order_bad(row, B, tid, nt)) {
    timed_bad_order<false>(out, B, T, 0, tid, nt);
    for (int k = tid; k < B; k += nt) order_out[k] = -1;
    if (tid == 0) { x.rounds_run[g] = 0; x.round_best[g] = -1; }
    return;
  }

  const TimedWork wk = timed_work_at<kLds>(work, g, q, T);
  // the row's slot and its two orders, behind the planner parts of all rows
  int *const slot_paths = (int *)(work + (size_t)gridDim.x * q.per_order + (size_t)g * timed_repair_words(T, B));
  int *const slot_status = slot_paths + (size_t)B * (T + 1), *const slot_arrive = slot_status + B;
  int *cur = slot_arrive + B, *next = cur + B;
  const TimedOut slot = {slot_status, slot_arrive, slot_paths, nullptr, nullptr, nullptr, nullptr};
  timed_free_mask(wk.freeb, p.grid, p.occ_threshold, d);
  for (int k = tid; k < B; k += nt) cur[k] = row[k];            // (the barriers of the first count cover both)
  const auto skipped = [&](int b) {
    const int s = p.start_cell[b], gi = p.goal_index[b];
    return s < 0 || s >= HW || gi < 0 || gi >= p.Gf;
  };
  TimedLaterStarts rule = {d, wk.cnt, wk.mask};

  long long best_key = INT64_MAX;
  int best_round = 0, r = 0;
  for (;; r++) {
    // a round starts from an empty table (stored as it is read and stamped: through the agent's atomics), the counts of
    // every start, and empty sums.  The loop over the ranks is k_timed_plan's, written out here a second time: as a
    // function of both kernels it cost k_timed_plan 2 % on the store.
    const TimedOut o = r == 0 ? out : slot;
    for (size_t i = tid; i < (size_t)(T + 1) * d.L; i += nt)
      __hip_atomic_store(wk.res + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    rule.count(cur, p.start_cell, B, skipped);
    TimedKey key;
    for (int k = 0; k < B; k++) {
      const int b = cur[k];
      int *const path = o.paths + (size_t)b * (T + 1);
      if (skipped(b)) {
        for (int t = tid; t <= T; t += nt) path[t] = -1;
        if (tid == 0) { o.status[b] = RMPC_GRID_OUTSIDE; o.arrive[b] = T + 1; key.skipped(T, 0, 0); }
        continue;
      }
      const int s = p.start_cell[b];
      rule.prepare(b, s);
      const TimedEnd e = timed_robot<false>(d, wk, rule, p.fields, p.goal_cells, s, 0, 0, nullptr, p.goal_index[b], 0, path,
                                            nullptr, o.status + b, o.arrive + b, red_d, red_c);
      if (tid == 0) key.planned(e.f, e.a, T, 0, 0);
    }
    if (tid == 0) round_key = key.key();
    __syncthreads();                                 // the key, and every status, arrive and path of the round
    const long long kr = round_key;
    if (r == 0 || kr < best_key) {                   // the least (key, round): a later round must be strictly better
      best_key = kr; best_round = r;
      if (r > 0) {
        for (size_t i = tid; i < (size_t)B * (T + 1); i += nt) out.paths[i] = slot_paths[i];
        for (int k = tid; k < B; k += nt) { out.status[k] = slot_status[k]; out.arrive[k] = slot_arrive[k]; }
      }
      for (int k = tid; k < B; k += nt) order_out[k] = cur[k];
      if (tid == 0) *out.key = kr;
    }
    if (r == x.rounds) break;
    bool changed;
    const int nbad = timed_repair_partition(cur, next, o.status, o.arrive, B, T, tid, nt, seg, changed);
    if (nbad == 0 || !changed) break;
    int *const was = cur;
    cur = next; next = was;
  }
  if (tid == 0) { x.rounds_run[g] = r + 1; x.round_best[g] = best_round; }
}

}  // namespace rmpc
