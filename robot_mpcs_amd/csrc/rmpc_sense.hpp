// rmpc_sense.hpp -- the lidar on the device (the reference's boxer examples: a Lidar sensor on the robot, then
// compute_point_cloud, then one free-space decomposition per stage around the previous plan), included by
// rmpc_host.hip.  The world is shared by all B robots: axis-aligned boxes [nbox][4] = (cx, cy, lx, ly) and circles
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
// Contraction is off: the kernels evaluate the restatement's expressions (tests/test_lidar_cpu.py).

namespace rmpc {

// sensor origin of the pose (x, y, th) with the body-frame offset (ox, oy); c, s = cos th, sin th
__device__ __forceinline__ void sense_origin(double x, double y, double c, double s, double ox, double oy, double &px,
                                             double &py) {
#pragma clang fp contract(off)
  px = x + ox * c - oy * s;
  py = y + ox * s + oy * c;
}

// One lane per (robot, ray): lane g = b * R + i, so with R = 64 one wavefront is one robot.  The shapes are read at
// wave-uniform addresses (every lane of a wave tests the same shape at the same time): the loads become scalar loads
// into SGPRs that the vector ALU reads directly.  Per box: two subtractions and two products per axis against the
// ray's reciprocal direction, min / max, no division.
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
  double *const o = points + (size_t)g * 3;
  o[0] = ox + t * dx;
  o[1] = oy + t * dy;
  o[2] = height;
  if (ranges) ranges[g] = t;
}

// One lane per (robot, stage): the sensor origin of q = z_prev [b][k][0 .. 2] (x_{k+1} of the previous plan, the
// reference's "Preprocessing for planner"), of the robot's current pose when there is no plan or its solve failed.
__global__ __launch_bounds__(256) void k_plan_points(const double *__restrict__ z_prev, int nvar,
                                                     const int *__restrict__ exitflag, const double *__restrict__ pose,
                                                     int stride, int B, int N, double offx, double offy, double height,
                                                     double *__restrict__ points) {
#pragma clang fp contract(off)
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= B * N) return;
  const int b = g / N;
  const bool plan = z_prev && !(exitflag && exitflag[b] < 0);
  const double *const q = plan ? z_prev + (size_t)g * nvar : pose + (size_t)b * stride;
  const double th = q[2];
  double ox, oy;
  sense_origin(q[0], q[1], cos(th), sin(th), offx, offy, ox, oy);
  double *const o = points + (size_t)g * 3;
  o[0] = ox;
  o[1] = oy;
  o[2] = height;
}

}  // namespace rmpc
