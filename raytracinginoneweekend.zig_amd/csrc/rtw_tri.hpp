// rtw_tri.hpp — the triangle primitive's arithmetic (rtw_hip.h RTW_PRIM_TRIANGLE,
// DESIGN.md §22), shared by the packer and the refit (the derived fields), the
// world kernels' root test and hit record (rtw_world_walk.hpp) and the host
// reference entry (rtw_world_trace_tri_host), so that none can drift from the
// others.  No HIP, no library calls: host and device; one IEEE operation per
// operator (the library builds with -ffp-contract=off); every sum in x, y, z
// order.
//
// Derived fields:  N = (v1 - v0) x (v2 - v0), n = N / sqrt(N . N) + 0.0 (a zero
// component is +0), h = n . v0.  Degenerate iff N . N is 0 or not finite.  For a
// triangle in the plane x_k = c, N has one non-zero component, sqrt(RN(x^2)) is
// |x| exactly, so n = +-e_k with +0 zeros and h = +-c.
//
// Root (the ray in object space):  t = (h - n . o) / (n . d); n . d == 0 (the ray
// lies in the plane) misses.  For n = +-e_k the zero products vanish and the
// signs cancel: the bits of the rect's (k - o_k) / d_k.
//
// Inside test, in ray space:  A = v0 - o, B = v1 - o, C = v2 - o,
//   w0 = d . (B x C), w1 = d . (C x A), w2 = d . (A x B);
// inside iff all three >= -tau_i or all three <= tau_i (zeros count on both
// sides; the test is two-sided).  p q - r s == -(r s - p q) and x + y ==
// -((-x) + (-y)) in floating point, so d . (P x Q) == -(d . (Q x P)) exactly:
// two triangles that share an edge with bit-identical vertices compute edge
// functions of exactly opposite sign for it, whatever their planes, and a ray
// between them is never rejected by both because of that edge.
// tau_i = 2^-49 (|dx| (|Py Qz| + |Pz Qy|) + |dy| (..) + |dz| (..)), the sum of
// the same six products' magnitudes: it bounds the rounding error of w_i (seven
// roundings per term, 7 u < 2^-50 relative to that sum).  The antisymmetry
// alone closes a mesh along its edges but not at its vertices: a ray through a
// vertex makes every edge function of the fan pure rounding noise, and all of
// them can come out with the same sign (tests/native/tri_check.cpp met it on
// 15 of ~10^4 vertex rays).  With tau, the triangle that holds the ray in exact
// arithmetic (all exact w_i >= 0, or all <= 0) is accepted whatever the
// rounding did, so a closed mesh is closed for every ray; a triangle grows by
// ~1e-15 of its size, and where two then overlap the list's tie rule decides.
// u = w1 / (w0 + w1 + w2), v = w2 / (w0 + w1 + w2): the barycentric weights of
// v1 and v2.
//
// Range: with every coordinate (vertices, origin, chain offsets) of magnitude
// <= 2^300 and 2^-300 <= |d| components' largest <= 2^300, the differences are
// <= 2^301, the products <= 2^602, the cross terms <= 2^603, the edge functions
// <= 3 * 2^903 and their sum <= 2^907: nothing overflows.  (An underflow to zero
// keeps the antisymmetry, so the mesh stays closed; only u, v lose accuracy.)
#pragma once

#if defined(__HIPCC__)
#define RTWT_HD __host__ __device__ inline
#else
#define RTWT_HD inline
#endif

namespace rtwtri {

// Where the thirteen doubles of a triangle live in its 16-double device record:
// v0, v1, v2 in doubles 0-8, n.x, n.y in 9-10, (11: the per-lane walk's kind
// copy,) n.z in 12, h in 13.
constexpr int kNx = 9, kNy = 10, kNz = 12, kH = 13;

// n and h of the triangle a = v0[3], v1[3], v2[3]; false: degenerate or not finite.
RTWT_HD bool derive(const double* a, double n[3], double& h) {
  const double e1x = a[3] - a[0], e1y = a[4] - a[1], e1z = a[5] - a[2];
  const double e2x = a[6] - a[0], e2y = a[7] - a[1], e2z = a[8] - a[2];
  const double Nx = e1y * e2z - e1z * e2y, Ny = e1z * e2x - e1x * e2z, Nz = e1x * e2y - e1y * e2x;
  const double nn = Nx * Nx + Ny * Ny + Nz * Nz;
  const double s = __builtin_sqrt(nn);
  n[0] = Nx / s + 0.0, n[1] = Ny / s + 0.0, n[2] = Nz / s + 0.0;
  h = n[0] * a[0] + n[1] * a[1] + n[2] * a[2];
  return nn - nn == 0.0 && nn != 0.0;
}

// The plane root; false when the ray lies in the plane.
RTWT_HD bool plane_t(double nx, double ny, double nz, double h, double ox, double oy, double oz, double dx, double dy,
                     double dz, double& t) {
  const double nd = nx * dx + ny * dy + nz * dz;
  if (nd == 0.0) return false;
  t = (h - (nx * ox + ny * oy + nz * oz)) / nd;
  return true;
}

// The three edge functions of the ray (o, d) against the vertices v[0..8].
RTWT_HD void edges(const double* v, double ox, double oy, double oz, double dx, double dy, double dz, double& w0,
                   double& w1, double& w2) {
  const double ax = v[0] - ox, ay = v[1] - oy, az = v[2] - oz;
  const double bx = v[3] - ox, by = v[4] - oy, bz = v[5] - oz;
  const double cx = v[6] - ox, cy = v[7] - oy, cz = v[8] - oz;
  w0 = dx * (by * cz - bz * cy) + dy * (bz * cx - bx * cz) + dz * (bx * cy - by * cx);
  w1 = dx * (cy * az - cz * ay) + dy * (cz * ax - cx * az) + dz * (cx * ay - cy * ax);
  w2 = dx * (ay * bz - az * by) + dy * (az * bx - ax * bz) + dz * (ax * by - ay * bx);
}
// d . (P x Q) and the bound tau of its rounding error (see the head of this file).
RTWT_HD double edge_tau(double px, double py, double pz, double qx, double qy, double qz, double dx, double dy,
                        double dz, double& tau) {
  const double yz = py * qz, zy = pz * qy, zx = pz * qx, xz = px * qz, xy = px * qy, yx = py * qx;
  tau = 0x1p-49 * (__builtin_fabs(dx) * (__builtin_fabs(yz) + __builtin_fabs(zy)) +
                   __builtin_fabs(dy) * (__builtin_fabs(zx) + __builtin_fabs(xz)) +
                   __builtin_fabs(dz) * (__builtin_fabs(xy) + __builtin_fabs(yx)));
  return dx * (yz - zy) + dy * (zx - xz) + dz * (xy - yx);
}
RTWT_HD bool inside(double w0, double w1, double w2, double t0, double t1, double t2) {
  return (w0 >= -t0 && w1 >= -t1 && w2 >= -t2) || (w0 <= t0 && w1 <= t1 && w2 <= t2);
}
// The inside test of the ray (o, d) against the vertices v[0..8].
RTWT_HD bool inside_ray(const double* v, double ox, double oy, double oz, double dx, double dy, double dz) {
  const double ax = v[0] - ox, ay = v[1] - oy, az = v[2] - oz;
  const double bx = v[3] - ox, by = v[4] - oy, bz = v[5] - oz;
  const double cx = v[6] - ox, cy = v[7] - oy, cz = v[8] - oz;
  double t0, t1, t2;
  const double w0 = edge_tau(bx, by, bz, cx, cy, cz, dx, dy, dz, t0);
  const double w1 = edge_tau(cx, cy, cz, ax, ay, az, dx, dy, dz, t1);
  const double w2 = edge_tau(ax, ay, az, bx, by, bz, dx, dy, dz, t2);
  return inside(w0, w1, w2, t0, t1, t2);
}

// The triangle's effective root for the object-space ray (o, d), as the other
// primitives' (rtw_world_walk.hpp root_obj): false when it cannot be hit at
// t >= tmin; t may be NaN.
RTWT_HD bool root(const double* v, double nx, double ny, double nz, double h, double ox, double oy, double oz,
                  double dx, double dy, double dz, double tmin, double& t) {
  double tt;
  if (!plane_t(nx, ny, nz, h, ox, oy, oz, dx, dy, dz, tt)) return false;
  if (tt < tmin) return false;
  if (!inside_ray(v, ox, oy, oz, dx, dy, dz)) return false;
  t = tt;
  return true;
}

// u, v of a hit: the weights of v1 and v2.
RTWT_HD void bary(const double* v, double ox, double oy, double oz, double dx, double dy, double dz, double& bu,
                  double& bv) {
  double w0, w1, w2;
  edges(v, ox, oy, oz, dx, dy, dz, w0, w1, w2);
  const double s = w0 + w1 + w2;
  bu = w1 / s, bv = w2 / s;
}

}  // namespace rtwtri
