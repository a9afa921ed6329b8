// rmpc_grid_large.hpp -- cost-to-go fields on maps beyond RMPC_GRID_MAX_CELLS (include/rmpc_grid_large.h, DESIGN.md
// 22), included by rmpc_world.hip behind rmpc_grid.hpp.  The recursion, the candidate delta + E(v) with
// E = cost_factor data + D, the strict minimum and the absence of contraction are those of grid_fields there, so the
// fixed point is the same bits; what differs is where the field lives.
//
// One workgroup per field, and no workgroup ever waits for another.  The field lives in fields [g] in global memory,
// which workgroup g alone reads and writes, and reads back only behind a __syncthreads(); one tile of kLargeTile x
// kLargeTile cells at a time lives in LDS, with the one-cell ring around it.  The work list is one flag bit per tile
// in LDS.  The rule (the header states it, tests/grid_large_reference.py restates it):
//   - D starts at +inf, 0 on the goal or the seed on seeded free cells; the tiles that hold a source start active, and
//     so do the tiles a source lies beside (a source is a cell lowered from +inf: without this a goal walled in on its
//     own tile but open towards the next one would never tell that tile);
//   - a visit clears the tile's flag, loads tile and ring (+inf outside the map), relaxes the tile's cells in place with
//     the ring held constant until a sweep lowers nothing (the tile's local fixed point, unique, so the order of the
//     sweeps inside the tile is free), stores the lowered cells back and flags every neighbouring tile beside which a
//     cell was lowered: the edge row or column for the 4 side neighbours, the corner cell for the 4 diagonal ones, which
//     count with 8 moves only;
//   - passes over the tiles, ascending index on even passes, descending on odd ones, visit every tile that is active
//     when it is reached; the loop ends with a pass that finds no flag.
// An inactive tile is at its local fixed point against its current ring, so one pass does at least one Jacobi step of
// the whole map: H W + 1 passes bound the loop, cells + 1 sweeps bound a visit (guards only, as in grid_fields).
//
// In LDS the tile is transposed, E(row, col) at col * kLargeStride + row: thread t owns the four cells (row t % 64,
// cols 4 (t / 64) .. + 3), so the 64 lanes of a wavefront read 64 consecutive doubles (no bank conflict) while a thread
// carries a value along its run of a row within one sweep, forwards on even sweeps and backwards on odd ones.  The
// stride is odd, which keeps the row-major fill (lanes along a row of the map, kLargeStride doubles apart in LDS) off
// shared bank pairs.

namespace rmpc {

constexpr int kLargeTile = RMPC_GRID_TILE;
constexpr int kLargeThreads = 1024;
constexpr int kLargeRun = kLargeTile * kLargeTile / kLargeThreads;   // cells per thread: a run along a row
constexpr int kLargeStride = kLargeTile + 3;                         // doubles per LDS column (tile + ring = T + 2)
// ceil(H / T) ceil(W / T) <= H W / T^2 + (H + W) / T + 1, and H + W is largest with one side at its limit
constexpr int kLargeMaxTiles = RMPC_GRID_LARGE_MAX_CELLS / (kLargeTile * kLargeTile) +
                               (RMPC_GRID_LARGE_MAX_SIDE + RMPC_GRID_LARGE_MAX_CELLS / RMPC_GRID_LARGE_MAX_SIDE) / kLargeTile + 2;
constexpr int kLargeFlagWords = (kLargeMaxTiles + 31) / 32;
static_assert(kLargeTile == 64 && kLargeRun == 4, "thread t owns row t % 64, columns 4 (t / 64) .. + 3");
static_assert(kLargeStride % 2 == 1, "odd LDS stride");

template <bool kSeeded>
__global__ __launch_bounds__(kLargeThreads) void k_grid_fields_large(const double *__restrict__ grid, int H, int W,
                                                                     const int *__restrict__ goal_cells,
                                                                     const double *__restrict__ seeds, int nmoves,
                                                                     double occ_threshold, double cost_factor,
                                                                     double *fields, int *__restrict__ status,
                                                                     int *__restrict__ visits_out) {
#pragma clang fp contract(off)
  __shared__ double E[(kLargeTile + 2) * kLargeStride];
  __shared__ unsigned flags[kLargeFlagWords];
  const int HW = H * W, g = blockIdx.x, t = threadIdx.x;
  const int ntx = (W + kLargeTile - 1) / kLargeTile, nty = (H + kLargeTile - 1) / kLargeTile, nt = ntx * nty;
  const int nwords = (nt + 31) / 32;
  const double inf = __builtin_inf();
  double *const F = fields + (size_t)g * HW;      // (not __restrict__: read back behind barriers)
  auto give_up = [&](int code) {
    for (int c = t; c < HW; c += kLargeThreads) F[c] = inf;
    if (t == 0) { status[g] = code; if (visits_out) visits_out[g] = 0; }
  };
  const int goal = kSeeded ? -1 : goal_cells[g];
  const bool goal_in = kSeeded || (goal >= 0 && goal < HW);
  const bool goal_ok = kSeeded || (goal_in && grid[goal] < occ_threshold);
  if (!goal_ok) { give_up(goal_in ? RMPC_GRID_GOAL_OCCUPIED : RMPC_GRID_OUTSIDE); return; }

  // the tiles a lowered cell (row lr, column lc of a tile of h x wd cells) wakes: bit (dr + 1) * 3 + dc + 1 for the
  // neighbour at (dr, dc); a tile one cell high or wide lies beside both neighbours of that direction
  auto beside = [&](int lr, int lc, int h, int wd) {
    const bool up = lr == 0, dn = lr == h - 1, lf = lc == 0, rt = lc == wd - 1, diag = nmoves == 8;
    return (up ? 2u : 0u) | (lf ? 8u : 0u) | (rt ? 32u : 0u) | (dn ? 128u : 0u) | (diag && up && lf ? 1u : 0u) |
           (diag && up && rt ? 4u : 0u) | (diag && dn && lf ? 64u : 0u) | (diag && dn && rt ? 256u : 0u);
  };
  auto raise = [&](int ty, int tx, unsigned wake) {
    for (int k = 0; k < 9; k++)
      if (wake & (1u << k)) {
        const int ny = ty + k / 3 - 1, nx = tx + k % 3 - 1;
        if (ny >= 0 && ny < nty && nx >= 0 && nx < ntx) {
          const int nb = ny * ntx + nx;
          atomicOr(&flags[nb >> 5], 1u << (nb & 31));
        }
      }
  };

  // D at its start, the checks of the map and the seeds, the flags of the tiles that hold a source and of those a
  // source lies beside (a source is a cell lowered from +inf to its seed)
  for (int w = t; w < kLargeFlagWords; w += kLargeThreads) flags[w] = 0u;
  __syncthreads();
  const double *const S = kSeeded ? seeds + (size_t)g * HW : nullptr;
  bool bad = false, bad_seed = false;
  for (int c = t; c < HW; c += kLargeThreads) {
    const double d = grid[c];
    const bool is_free = d < occ_threshold;
    bad = bad || (is_free && !(d >= 0.0));
    double v = inf;
    if constexpr (kSeeded) {
      v = is_free ? S[c] : inf;                   // a seed on an occupied cell is ignored
      bad_seed = bad_seed || !(v >= 0.0);
    } else if (c == goal) {
      v = 0.0;
    }
    F[c] = v;
    if (v < inf) {
      const int r = c / W, col = c - r * W, ty = r / kLargeTile, tx = col / kLargeTile;
      raise(ty, tx, 16u | beside(r - ty * kLargeTile, col - tx * kLargeTile, min(kLargeTile, H - ty * kLargeTile),
                                 min(kLargeTile, W - tx * kLargeTile)));
    }
  }
  if (__syncthreads_or(bad)) { give_up(RMPC_GRID_BAD_MAP); return; }
  if constexpr (kSeeded) {
    if (__syncthreads_or(bad_seed)) { give_up(RMPC_GRID_BAD_SEED); return; }
  }

  const int lr = t & (kLargeTile - 1), lc0 = (t / kLargeTile) * kLargeRun;    // this thread's cells within a tile
  double *const Et = E + (lc0 + 1) * kLargeStride + lr + 1;
  long long visits = 0;
  bool converged = true, done = false;
  for (int pass = 0; !done && converged; pass++) {
    if (pass > HW) { converged = false; break; }
    const bool down = pass & 1;
    bool visited = false;
    for (int wi = 0; wi < nwords && converged; wi++) {
      const int w = down ? nwords - 1 - wi : wi;
      unsigned seen = 0u;                         // the bits of this word the pass is past
      for (;;) {
        // one value in every thread: the flags rest between the last barrier of a visit and the first of the next
        const unsigned word = __builtin_amdgcn_readfirstlane(flags[w]) & ~seen;
        if (!word) break;
        const int b = down ? 31 - __clz(word) : __ffs(word) - 1;
        seen |= down ? ~((1u << b) - 1u) : (b == 31 ? ~0u : (2u << b) - 1u);
        const int tile = w * 32 + b, ty = tile / ntx, tx = tile - ty * ntx;
        const int r0 = ty * kLargeTile, c0 = tx * kLargeTile;
        const int h = min(kLargeTile, H - r0), wd = min(kLargeTile, W - c0);
        visited = true;
        visits++;
        // the tile and its ring, row-major over the map: E = cost_factor data + D on free cells, +inf elsewhere
        for (int i = t; i < (h + 2) * (wd + 2); i += kLargeThreads) {
          const int rr = i / (wd + 2), cc = i - rr * (wd + 2), r = r0 - 1 + rr, c = c0 - 1 + cc;
          double e = inf;
          if (r >= 0 && r < H && c >= 0 && c < W) {
            const double d = grid[r * W + c];
            if (d < occ_threshold) e = cost_factor * d + F[r * W + c];
          }
          E[cc * kLargeStride + rr] = e;
        }
        // this thread's cells: D, the price and whether the cell takes part (inside the tile and free)
        double D[kLargeRun], D0[kLargeRun], price[kLargeRun];
        unsigned part = 0u;
#pragma unroll
        for (int i = 0; i < kLargeRun; i++) {
          D[i] = D0[i] = inf;
          price[i] = 0.0;
          if (lr < h && lc0 + i < wd) {
            const int c = (r0 + lr) * W + c0 + lc0 + i;
            const double d = grid[c];
            if (d < occ_threshold) {
              part |= 1u << i;
              price[i] = cost_factor * d;
              D[i] = D0[i] = F[c];
            }
          }
        }
        __syncthreads();
        if (t == 0) atomicAnd(&flags[w], ~(1u << b));
        auto relax = [&](int i, bool &lowered) {
          if (part & (1u << i)) {
            const double *const e = Et + i * kLargeStride;
            double best = D[i];
            const double c0_ = grid_delta(0) + e[kLargeStride], c1_ = grid_delta(1) + e[1];
            const double c2_ = grid_delta(2) + e[-kLargeStride], c3_ = grid_delta(3) + e[-1];
            best = c0_ < best ? c0_ : best;
            best = c1_ < best ? c1_ : best;
            best = c2_ < best ? c2_ : best;
            best = c3_ < best ? c3_ : best;
            if (nmoves == 8) {
              const double c4_ = grid_delta(4) + e[kLargeStride + 1], c5_ = grid_delta(5) + e[-kLargeStride + 1];
              const double c6_ = grid_delta(6) + e[-kLargeStride - 1], c7_ = grid_delta(7) + e[kLargeStride - 1];
              best = c4_ < best ? c4_ : best;
              best = c5_ < best ? c5_ : best;
              best = c6_ < best ? c6_ : best;
              best = c7_ < best ? c7_ : best;
            }
            if (best < D[i]) {
              D[i] = best;
              Et[i * kLargeStride] = price[i] + best;
              lowered = true;
            }
          }
        };
        int sweep = 0;
        bool quiet = false;
        for (; sweep <= h * wd; sweep++) {
          bool lowered = false;
          if (sweep & 1) {
#pragma unroll
            for (int i = kLargeRun - 1; i >= 0; i--) relax(i, lowered);
          } else {
#pragma unroll
            for (int i = 0; i < kLargeRun; i++) relax(i, lowered);
          }
          if (!__syncthreads_or(lowered)) { quiet = true; break; }
        }
        if (!quiet) converged = false;
        // the lowered cells go back, and wake the tiles they lie beside
        unsigned wake = 0u;
#pragma unroll
        for (int i = 0; i < kLargeRun; i++)
          if (D[i] < D0[i]) {
            F[(r0 + lr) * W + c0 + lc0 + i] = D[i];
            wake |= beside(lr, lc0 + i, h, wd);
          }
        if (wake) raise(ty, tx, wake);
        __syncthreads();
        if (!converged) break;
      }
    }
    done = !visited;
  }
  if (!converged) { __syncthreads(); give_up(RMPC_GRID_NO_FIXED_POINT); return; }
  if (t == 0) {
    status[g] = RMPC_GRID_OK;
    if (visits_out) visits_out[g] = visits > INT_MAX ? INT_MAX : (int)visits;
  }
}

}  // namespace rmpc
