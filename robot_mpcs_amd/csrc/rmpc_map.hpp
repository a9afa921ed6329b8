// rmpc_map.hpp -- the fleet's occupancy evidence on the device: lidar scans marked into two int32 count grids and the
// counts classified into the occupancy grid the global planner reads, included by rmpc_world.hip.
// Grids are [H][W], row-major, in the planner's plain frame: cell (row, col) is centred at (x0 + col cell, y0 + row cell).
//
// One ray (b, i), o = origins [b][0 .. 1], e = points [b][i][0 .. 1], t = ranges [b][i]; every expression in this order:
//   1. skipped unless o, e, t are finite and 0 < t <= range;
//   2. hit = t < range; then s = hit_depth / t, e <- e + s (e - o): the end cell is taken hit_depth behind the face;
//   3. ua = (ox - x0) / cell + 0.5, va, ub, vb likewise; (c, r) = floor (ua, va), (c1, r1) = floor (ub, vb),
//      n = |c1 - c| + |r1 - r|; skipped unless n <= 2 ceil((range + hit_depth) / cell) + 4 (false for a NaN as well);
//   4. du = ub - ua, sc = du > 0 ? 1 : -1, tx = du != 0 ? ((c + (du > 0 ? 1 : 0)) - ua) / du : +inf; dv, sr, ty likewise;
//   5. n + 1 cells from (r, c): misses += 1 on a cell inside the map, hits += 1 instead on the last cell of a hit;
//      between two visits the column steps (c += sc, tx from the new c) when (tx <= ty and c != c1) or r == r1, else
//      the row.  The walk (Amanatides & Woo) moves towards (r1, c1) in both coordinates and ends there.
// Contraction is off: the kernels evaluate the restatement's expressions (tests/mapping_reference.py), and the counts
// are integers, so a map is bitwise the same whatever the order of the adds.

namespace rmpc {

struct MapGeom {
  int H, W;
  double x0, y0, cell, range, hit_depth;
  double nmax;   // 2 ceil((range + hit_depth) / cell) + 4, at most 2^30 (checked by the entry)
};

struct MapRay {
  int c, r, c1, r1, n;
  double ua, va, du, dv;
  bool hit;
};

__device__ __forceinline__ double map_coord(double p, double p0, double cell) {
#pragma clang fp contract(off)
  return (p - p0) / cell + 0.5;
}

// steps 1 - 3: -1 the ray is skipped, 0 it adds nothing (the box spanned by its end cells misses the map, and the
// walk never leaves that box), 1 walk it.  After 1, all four cell coordinates fit an int: n <= 2^30 and a coordinate
// of each pair lies within the map.
__device__ __forceinline__ int map_ray(const double *o, const double *e, double t, const MapGeom &g, MapRay &q) {
#pragma clang fp contract(off)
  const double ox = o[0], oy = o[1];
  double ex = e[0], ey = e[1];
  if (!(isfinite(ox) && isfinite(oy) && isfinite(ex) && isfinite(ey) && isfinite(t) && t > 0.0 && t <= g.range)) return -1;
  q.hit = t < g.range;
  if (q.hit) {
    const double s = g.hit_depth / t;
    ex = ex + s * (ex - ox);
    ey = ey + s * (ey - oy);
  }
  q.ua = map_coord(ox, g.x0, g.cell);
  q.va = map_coord(oy, g.y0, g.cell);
  const double ub = map_coord(ex, g.x0, g.cell), vb = map_coord(ey, g.y0, g.cell);
  const double c = floor(q.ua), r = floor(q.va), c1 = floor(ub), r1 = floor(vb);
  const double n = fabs(c1 - c) + fabs(r1 - r);
  if (!(n <= g.nmax)) return -1;
  if (fmax(c, c1) < 0.0 || fmin(c, c1) >= (double)g.W || fmax(r, r1) < 0.0 || fmin(r, r1) >= (double)g.H) return 0;
  q.c = (int)c; q.r = (int)r; q.c1 = (int)c1; q.r1 = (int)r1; q.n = (int)n;
  q.du = ub - q.ua;
  q.dv = vb - q.va;
  return 1;
}

// steps 4 - 5: visit(row, col, is_hit) for every visited cell inside the map
template <class Visit>
__device__ __forceinline__ void map_walk(const MapRay &q, int H, int W, Visit &&visit) {
#pragma clang fp contract(off)
  const double inf = __builtin_inf();
  const int pc = q.du > 0.0 ? 1 : 0, pr = q.dv > 0.0 ? 1 : 0;
  const int sc = pc ? 1 : -1, sr = pr ? 1 : -1;
  int c = q.c, r = q.r;
  double tx = q.du != 0.0 ? ((double)(c + pc) - q.ua) / q.du : inf;
  double ty = q.dv != 0.0 ? ((double)(r + pr) - q.va) / q.dv : inf;
  for (int k = 0;; k++) {
    if ((unsigned)r < (unsigned)H && (unsigned)c < (unsigned)W) visit(r, c, q.hit && k == q.n);
    if (k == q.n) break;
    if ((tx <= ty && c != q.c1) || r == q.r1) {
      c += sc;
      tx = ((double)(c + pc) - q.ua) / q.du;   // (a column step implies c != c1, hence du != 0)
    } else {
      r += sr;
      ty = ((double)(r + pr) - q.va) / q.dv;
    }
  }
}

// One lane per (robot, ray), every visit a global atomic on the int32 counters.
__global__ __launch_bounds__(256) void k_grid_mark(const double *__restrict__ origins, const double *__restrict__ points,
                                                   const double *__restrict__ ranges, int B, int R, MapGeom g,
                                                   int *__restrict__ hits, int *__restrict__ misses,
                                                   int *__restrict__ skipped) {
#pragma clang fp contract(off)
  const int gi = blockIdx.x * 256 + threadIdx.x;
  if (gi >= B * R) return;
  const int b = gi / R, W = g.W;
  MapRay q;
  const int s = map_ray(origins + (size_t)b * 3, points + (size_t)gi * 3, ranges[gi], g, q);
  if (s < 0 && skipped) atomicAdd(skipped, 1);
  if (s > 0) map_walk(q, g.H, W, [&](int r, int c, bool h) { atomicAdd((h ? hits : misses) + r * W + c, 1); });
}

// One lane per cell: the class of the cell from its counts, then the ageing shift
__global__ __launch_bounds__(256) void k_grid_occupancy(int n, int *__restrict__ hits, int *__restrict__ misses, int w_hit,
                                                        int w_miss, int forget, double free_value, double occ_value,
                                                        double unknown_value, double *__restrict__ grid) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int h = hits[i], m = misses[i];
  grid[i] = (long long)h + (long long)m == 0 ? unknown_value
            : ((long long)h * w_hit > (long long)m * w_miss ? occ_value : free_value);
  if (forget > 0) {
    hits[i] = h >> forget;
    misses[i] = m >> forget;
  }
}

// One lane per cell: the planning grid and the frontier of the map.  known(c) = hits + misses != 0, the
// rule of k_grid_occupancy; plan = the enlarged grid on known cells and unknown_value elsewhere (the unknown region is
// not dilated: that would block every frontier cell); a frontier cell is known, free on the enlarged grid and has a
// neighbour inside the map without evidence; seed = 0 there, +inf elsewhere.  *count grows by the number of frontier
// cells, one integer atomicAdd per workgroup that holds any: the sum does not depend on the order.
__global__ __launch_bounds__(256) void k_grid_frontier(int H, int W, const int *__restrict__ hits, const int *__restrict__ misses,
                                                       const double *__restrict__ enlarged, double occ_threshold, int nmoves,
                                                       double unknown_value, double *__restrict__ plan,
                                                       double *__restrict__ seed, int *__restrict__ count) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * 256 + threadIdx.x;
  bool frontier = false;
  if (c < H * W) {
    const bool known = (long long)hits[c] + (long long)misses[c] != 0;
    const double e = enlarged[c];
    plan[c] = known ? e : unknown_value;
    if (known && e < occ_threshold) {
      const int r = c / W, col = c - r * W;
      for (int m = 0; m < nmoves; m++) {
        const int rr = r + grid_dr(m), cc = col + grid_dc(m);
        if (rr < 0 || rr >= H || cc < 0 || cc >= W) continue;
        const int v = rr * W + cc;
        frontier = frontier || (long long)hits[v] + (long long)misses[v] == 0;
      }
    }
    seed[c] = frontier ? 0.0 : __builtin_inf();
  }
  const int n = __syncthreads_count(frontier);
  if (threadIdx.x == 0 && n > 0) atomicAdd(count, n);
}

}  // namespace rmpc
