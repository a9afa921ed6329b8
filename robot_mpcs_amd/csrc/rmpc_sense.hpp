// rmpc_sense.hpp -- the lidar on the device (the reference's boxer examples: a Lidar sensor on the robot, then
// compute_point_cloud, then one free-space decomposition per stage around the previous plan), included by
// rmpc_world.hip.  The world is shared by all B robots: axis-aligned boxes [nbox][4] = (cx, cy, lx, ly) and circles
// [ncircle][3] = (cx, cy, r).  The ray convention is the project's own ("Lidar"):
//   sensor origin  o = (x + ox cos th - oy sin th, y + ox sin th + oy cos th), (ox, oy) in the body frame;
//   ray i of R     angle th + a_min + i (a_max - a_min) / R (half-open sweep), direction d = (cos, sin);
//   boxes          slab test, hit = entering distance t_enter with 0 < t_enter <= t_exit; a direction component that
//                  is exactly 0 never divides: the ray is inside that slab iff the origin coordinate lies in the
//                  closed interval;
//   circles        t = -b - sqrt(b^2 - c), b = d.(o - c), c = |o - c|^2 - r^2; a hit iff c > 0, b^2 - c >= 0, t > 0;
//   a shape that contains the origin is ignored by that ray (t_enter <= 0, c <= 0): FSD would otherwise get a point
//   at its own seed, a plane with normal 0;
//   t              the least hit distance, range when nothing is hit within range.
// Contraction is off: the kernels evaluate the restatement's expressions (tests/lidar_reference.py).
// The fleet's separating planes (k_fleet_planes, below) live here too: their points come from k_plan_points.

namespace rmpc {

// sensor origin of the pose (x, y, th) with the body-frame offset (ox, oy); c, s = cos th, sin th
__device__ __forceinline__ void sense_origin(double x, double y, double c, double s, double ox, double oy, double &px,
                                             double &py) {
#pragma clang fp contract(off)
  px = x + ox * c - oy * s;
  py = y + ox * s + oy * c;
}

// The least hit distance of the ray (o, d) in the static world, range when nothing is hit within range.  The shapes
// are read at wave-uniform addresses (every lane of a wave tests the same shape at the same time): the loads become
// scalar loads into SGPRs that the vector ALU reads directly.  Per box: two subtractions and two products per axis
// against the ray's reciprocal direction, min / max, no division.  One copy for k_lidar and k_lidar_fleet: the fleet
// scan's static_ranges are the plain scan's ranges bit for bit.
__device__ __forceinline__ double lidar_static(double ox, double oy, double dx, double dy, double range,
                                               const double *__restrict__ boxes, int nbox,
                                               const double *__restrict__ circles, int ncircle) {
#pragma clang fp contract(off)
  const bool zx = dx == 0.0, zy = dy == 0.0;
  const double ix = zx ? 0.0 : 1.0 / dx, iy = zy ? 0.0 : 1.0 / dy;
  const double inf = __builtin_inf();
  double t = range;
  for (int j = 0; j < nbox; j++) {
    const double *const q = boxes + 4 * j;
    const double hx = 0.5 * q[2], hy = 0.5 * q[3];
    const double x0 = q[0] - hx, x1 = q[0] + hx, y0 = q[1] - hy, y1 = q[1] + hy;
    const double ax = (x0 - ox) * ix, bx = (x1 - ox) * ix;
    const double ay = (y0 - oy) * iy, by = (y1 - oy) * iy;
    double nx = fmin(ax, bx), fx = fmax(ax, bx), ny = fmin(ay, by), fy = fmax(ay, by);
    if (zx) { nx = ox >= x0 && ox <= x1 ? -inf : inf; fx = inf; }
    if (zy) { ny = oy >= y0 && oy <= y1 ? -inf : inf; fy = inf; }
    const double te = fmax(nx, ny), tx = fmin(fx, fy);
    if (te > 0.0 && te <= tx && te < t) t = te;
  }
  for (int j = 0; j < ncircle; j++) {
    const double *const q = circles + 3 * j;
    const double ux = ox - q[0], uy = oy - q[1];
    const double bb = dx * ux + dy * uy;
    const double cc = (ux * ux + uy * uy) - q[2] * q[2];
    const double disc = bb * bb - cc;
    if (cc > 0.0 && disc >= 0.0) {
      const double tc = -bb - sqrt(disc);
      if (tc > 0.0 && tc < t) t = tc;
    }
  }
  return t;
}

// One lane per (robot, ray): lane g = b * R + i, so with R = 64 one wavefront is one robot.
__global__ __launch_bounds__(256) void k_lidar(const double *__restrict__ pose, int stride, int B, int R, double amin,
                                               double step, double range, double offx, double offy, double height,
                                               const double *__restrict__ boxes, int nbox,
                                               const double *__restrict__ circles, int ncircle,
                                               double *__restrict__ points, double *__restrict__ ranges) {
#pragma clang fp contract(off)
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= B * R) return;
  const int b = g / R, i = g - b * R;
  const double *const p = pose + (size_t)b * stride;
  const double x = p[0], y = p[1], th = p[2];
  double ox, oy;
  sense_origin(x, y, cos(th), sin(th), offx, offy, ox, oy);
  const double ang = (th + amin) + (double)i * step;
  const double dx = cos(ang), dy = sin(ang);
  const double t = lidar_static(ox, oy, dx, dy, range, boxes, nbox, circles, ncircle);
  double *const o = points + (size_t)g * 3;
  o[0] = ox + t * dx;
  o[1] = oy + t * dy;
  o[2] = height;
  if (ranges) ranges[g] = t;
}

// ---- the fleet in the scan: the static world of k_lidar plus P round bodies, one per robot --------
// One workgroup per scanning robot b, its lanes sharing the rays (a batch of blockDim.x rays at a time).  A ray first
// takes its static hit ts from lidar_static.  The bodies then pass in chunks of blockDim.x: each lane holds one body
// against the cull (not the robot's own, radius > 0, |o - c|^2 <= (range + r)^2 with a relative margin of 1e-6, about
// 1e10 rounding errors: a body outside it has tc > range for every ray); a 64-bit ballot and a popcount compact the
// survivors of a wave, the waves' counts meet in LDS, and the survivors go to an LDS list of (cx, cy, r, j).  When the
// next chunk might not fit, every lane tests its ray against the list (all lanes read the same entry at the same time: a
// broadcast) and the list starts again, so there is no limit on the bodies in range.  The ray keeps the least (tc, j)
// with tc < ts strictly: a minimum with an index tie-break, so the result does not depend on the order in which the
// bodies are met.  A NaN centre or radius fails the cull as it would fail the rule.
constexpr int kFleetListMax = 512;   // entries of the LDS list; >= the largest block (256)

__global__ __launch_bounds__(256) void k_lidar_fleet(const double *__restrict__ pose, int stride, int R, double amin,
                                                     double step, double range, double offx, double offy, double height,
                                                     const double *__restrict__ boxes, int nbox,
                                                     const double *__restrict__ circles, int ncircle,
                                                     const double *__restrict__ centres, int cstride,
                                                     const double *__restrict__ radius, int P, int self0,
                                                     double *__restrict__ points, double *__restrict__ ranges,
                                                     double *__restrict__ static_ranges, int *__restrict__ owner) {
#pragma clang fp contract(off)
  __shared__ double lx[kFleetListMax], ly[kFleetListMax], lr[kFleetListMax];
  __shared__ int lj[kFleetListMax];
  __shared__ int wc[4];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int wave = tid >> 6, lane = tid & 63, nw = nt >> 6;
  const double *const p = pose + (size_t)b * stride;
  const double x = p[0], y = p[1], th = p[2];
  double ox, oy;
  sense_origin(x, y, cos(th), sin(th), offx, offy, ox, oy);
  const long long self = (long long)self0 + b;
  for (int i0 = 0; i0 < R; i0 += nt) {
    const int i = i0 + tid;
    const double ang = (th + amin) + (double)i * step;
    const double dx = cos(ang), dy = sin(ang);
    const double ts = lidar_static(ox, oy, dx, dy, range, boxes, nbox, circles, ncircle);
    double t = ts;
    int own = -1;
    // the ray against the n entries of the list
    auto drain = [&](int n) {
      for (int e = 0; e < n; e++) {
        const double r = lr[e];
        const int j = lj[e];
        const double ux = ox - lx[e], uy = oy - ly[e];
        const double bb = dx * ux + dy * uy;
        const double cc = (ux * ux + uy * uy) - r * r;
        const double disc = bb * bb - cc;
        if (cc > 0.0 && disc >= 0.0) {
          const double tc = -bb - sqrt(disc);
          if (tc > 0.0 && (tc < t || (tc == t && own >= 0 && j < own))) { t = tc; own = j; }
        }
      }
    };
    int count = 0;   // the same in every lane of the block
    for (int j0 = 0; j0 < P; j0 += nt) {
      if (count + nt > kFleetListMax) { drain(count); count = 0; }
      const int j = j0 + tid;
      double cx = 0.0, cy = 0.0, r = 0.0;
      bool keep = false;
      if (j < P && (long long)j != self) {
        const double *const c = centres + (size_t)j * cstride;
        cx = c[0]; cy = c[1]; r = radius[j];
        const double ux = ox - cx, uy = oy - cy, lim = range + r;
        keep = r > 0.0 && ux * ux + uy * uy <= (lim * lim) * 1.000001;
      }
      const unsigned long long m = __ballot(keep);
      if (lane == 0) wc[wave] = __popcll(m);
      __syncthreads();
      int at = count;
      for (int w = 0; w < nw; w++) {
        const int n = wc[w];
        if (w < wave) at += n;
        count += n;
      }
      if (keep) {
        at += __popcll(m & ((1ull << lane) - 1ull));
        lx[at] = cx; ly[at] = cy; lr[at] = r; lj[at] = j;
      }
      __syncthreads();
    }
    drain(count);
    if (i < R) {
      const size_t g = (size_t)b * R + i;
      double *const o = points + g * 3;
      o[0] = ox + t * dx;
      o[1] = oy + t * dy;
      o[2] = height;
      if (ranges) ranges[g] = t;
      if (static_ranges) static_ranges[g] = ts;
      if (owner) owner[g] = own >= 0 ? own : (ts < range ? -2 : -1);
    }
  }
}

// One lane per (robot, stage): the sensor origin of q = z_prev [b][k][0 .. 2] (x_{k+1} of the previous plan, the
// reference's "Preprocessing for planner"), of the robot's current pose when there is no plan or its solve failed.
// shift = 1 reads stage min(k + 1, N - 1) instead (the coming solve's stage k, the last stage held: the fleet's
// predicted collision points); heading = 0 writes (q0, q1, height) without the sensor offset (the point robot).
__global__ __launch_bounds__(256) void k_plan_points(const double *__restrict__ z_prev, int nvar,
                                                     const int *__restrict__ exitflag, const double *__restrict__ pose,
                                                     int stride, int B, int N, int shift, int heading, double offx,
                                                     double offy, double height, double *__restrict__ points) {
#pragma clang fp contract(off)
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= B * N) return;
  const int b = g / N;
  const int k = g - b * N;
  const int kk = shift ? min(k + 1, N - 1) : k;
  const bool plan = z_prev && !(exitflag && exitflag[b] < 0);
  const double *const q = plan ? z_prev + ((size_t)b * N + kk) * nvar : pose + (size_t)b * stride;
  double *const o = points + (size_t)g * 3;
  if (heading) {
    const double th = q[2];
    double ox, oy;
    sense_origin(q[0], q[1], cos(th), sin(th), offx, offy, ox, oy);
    o[0] = ox;
    o[1] = oy;
  } else {
    o[0] = q[0];
    o[1] = q[1];
  }
  o[2] = height;
}

// ---- fleet separation: one separating plane per neighbour pair and stage ------------------------
// Robot b at stage k with q_j = points [j][k]: the candidates are j != b with s_j = (u0^2 + u1^2) + u2^2 < range^2,
// u = q_j - q_b; the K of least s_j (ties to the lower j) go to slots slot0 .. slot0 + K - 1 of planes [b][k][nobst].
// The plane of a pair is computed from the lower index lo and the higher hi, so both robots hold bitwise-negated
// copies of it: u = q_lo - q_hi, d = |u|, n = u / d ((1, 0, 0) when d = 0), g = d - r_lo - r_hi (the free gap),
// m = q_hi + (r_hi + g / 2) n, c = -n.m; robot lo gets (n, c), robot hi (-n, -c).  Slots without a candidate get
// k_fsd's dummy plane around q_b.
constexpr int kFleetKMax = 8;

// All-pairs scan in the shape of an N-body tiling: one block = 256 robots at one stage; tiles of 256 candidates pass
// through LDS and every lane reads the same LDS word at the same time (a broadcast).  The sorted top-K list stays in
// registers (kFleetKMax slots, fully unrolled; slots >= K hold -inf so that nothing enters them), the robot's own entry
// gets s = +inf instead of a branch.  `worst` = the K-th least s so far (range^2 while the list is not full): a
// candidate enters iff s < worst, which also keeps equal s in the order of j.
__global__ __launch_bounds__(256) void k_fleet_planes(const double *__restrict__ points,
                                                      const double *__restrict__ radius, int B, int N, int K,
                                                      double r2, int nobst, int slot0, double *__restrict__ planes) {
#pragma clang fp contract(off)
  __shared__ double tx[256], ty[256], tz[256];
  const int nbt = (B + 255) / 256;
  const int k = blockIdx.x / nbt;
  const int b = (blockIdx.x - k * nbt) * 256 + threadIdx.x;
  const bool live = b < B;
  const double *const qb = points + ((size_t)(live ? b : B - 1) * N + k) * 3;
  const double x = qb[0], y = qb[1], z = qb[2];
  const double inf = __builtin_inf();
  double ts[kFleetKMax];
  int tj[kFleetKMax];
#pragma unroll
  for (int i = 0; i < kFleetKMax; i++) {
    ts[i] = i < K ? r2 : -inf;
    tj[i] = -1;
  }
  double worst = r2;
  for (int j0 = 0; j0 < B; j0 += 256) {
    __syncthreads();
    {
      // a tile holds 256 candidates; the entries past B sit at +inf, where s = +inf never enters the list
      const bool in = j0 + (int)threadIdx.x < B;
      const double *const q = points + ((size_t)(in ? j0 + threadIdx.x : 0) * N + k) * 3;
      tx[threadIdx.x] = in ? q[0] : inf;
      ty[threadIdx.x] = in ? q[1] : inf;
      tz[threadIdx.x] = in ? q[2] : inf;
    }
    __syncthreads();
    for (int t = 0; t < 256; t++) {
      const double u0 = tx[t] - x, u1 = ty[t] - y, u2 = tz[t] - z;
      const double s = j0 + t == b ? inf : (u0 * u0 + u1 * u1) + u2 * u2;
      if (s < worst) {
        // sorted insert by (s, j): the new candidate has the largest j so far and goes behind equal s; an entry it
        // displaces keeps its place before the equal s behind it
        double cs = s;
        int cj = j0 + t;
#pragma unroll
        for (int i = 0; i < kFleetKMax; i++) {
          const bool lt = cs < ts[i] || (cs == ts[i] && cj < tj[i]);
          const double os = ts[i];
          const int oj = tj[i];
          ts[i] = lt ? cs : os;
          tj[i] = lt ? cj : oj;
          cs = lt ? os : cs;
          cj = lt ? oj : cj;
        }
        worst = ts[0];
#pragma unroll
        for (int i = 1; i < kFleetKMax; i++) worst = fmax(worst, ts[i]);
      }
    }
  }
  if (!live) return;
  const double rb = radius[b];
  double *const o = planes + (((size_t)b * N + k) * nobst + slot0) * 4;
#pragma unroll
  for (int i = 0; i < kFleetKMax; i++) {
    if (i >= K) break;
    const int j = tj[i];
    double n0, n1, n2, c;
    if (j < 0) {
      // HalfPlane(seed + (20, 20, 0), seed) of k_fsd: normal = seed - point
      const double p0 = x + 20.0, p1 = y + 20.0, p2 = z + 0.0;
      n0 = x - p0; n1 = y - p1; n2 = z - p2;
      c = -((n0 * p0 + n1 * p1) + n2 * p2);
    } else {
      const double *const qj = points + ((size_t)j * N + k) * 3;
      const double rj = radius[j];
      const bool lo = b < j;
      const double l0 = lo ? x : qj[0], l1 = lo ? y : qj[1], l2 = lo ? z : qj[2], rl = lo ? rb : rj;
      const double h0 = lo ? qj[0] : x, h1 = lo ? qj[1] : y, h2 = lo ? qj[2] : z, rh = lo ? rj : rb;
      const double u0 = l0 - h0, u1 = l1 - h1, u2 = l2 - h2;
      const double d = sqrt((u0 * u0 + u1 * u1) + u2 * u2);
      const bool z0 = d == 0.0;
      n0 = z0 ? 1.0 : u0 / d;
      n1 = z0 ? 0.0 : u1 / d;
      n2 = z0 ? 0.0 : u2 / d;
      const double g = (d - rl) - rh;
      const double w = rh + 0.5 * g;
      const double m0 = h0 + w * n0, m1 = h1 + w * n1, m2 = h2 + w * n2;
      c = -((n0 * m0 + n1 * m1) + n2 * m2);
      if (!lo) { n0 = -n0; n1 = -n1; n2 = -n2; c = -c; }
    }
    o[4 * i] = n0;
    o[4 * i + 1] = n1;
    o[4 * i + 2] = n2;
    o[4 * i + 3] = c;
  }
}

}  // namespace rmpc
