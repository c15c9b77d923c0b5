// rtw_beam.hpp — conservative bound: which spheres can a tile's camera rays hit?
//
// Camera.getRay (main.zig:91-100) starts a ray at O' = O + R_l (dx cu + dy cv),
// (dx, dy) in the unit disk, towards Q = llc + s horizontal + t vertical on the
// focus plane; its points are (1 - l) O' + l Q, l >= 0, and a root of
// Sphere.hit IS that l (the direction Q - O' is not normalised).  All camera
// rays of one 8x8-pixel tile — every sample, jitter, lens point and shutter
// time — have O' in the lens disk (centre O, radius R) and Q in the tile's
// parallelogram on the focus plane (centre Qc, half-diagonal h), so the ray
// point at parameter l lies within
//     rho(l) = |1 - l| R + l h
// of the axis point A(l) = O + l (Qc - O).  A sphere (C, r) can be hit at some
// l >= 0 only if |A(l) - C| <= |r| + rho(l) for that l (the ball, not only its
// surface: a camera inside the sphere is covered at l = 0).  rho is linear on
// [0, 1] and on [1, inf), so on each piece the test is the sign of the minimum
// of a quadratic in l:
//     g(l) = |E + l D|^2 - (alpha + beta l)^2,   E = O - C, D = Qc - O.
// A moving sphere is bounded by the sphere that covers its travel over the
// camera's shutter interval.  Everything is f64 with an outward margin (kRel
// on every radius and on the final comparison, ~10^6 times the rounding of
// these operations and of the kernel's exact test), and every comparison is
// written so that a NaN or an infinity answers "may be hit".  A beam whose
// cone is wider than ~45 degrees (the quadratic's leading coefficient not
// safely positive) answers "may be hit" as well.
// The megakernel evaluates the bound once per 64-unit batch, lane j for
// clustered slot j (rtw_trace.hip take_units); tests/test_beam_host.py checks
// it against exact solves of rays at the extremes of every tile.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RTWB_HD __host__ __device__ __forceinline__
#else
#define RTWB_HD inline
#endif

namespace rtwb {

constexpr double kRel = 1e-9;  // outward margin (relative)

// The tile's beam: axis O + l D, lens-disk radius R, focus-quad half-diagonal h.
struct Beam {
  double O[3], D[3], DD, R, h;
};

// px0..px1: the tile's pixel columns; y0..y1: its image rows (top-first, the
// min and max of row_begin + ly * row_stride over the tile's ly); W, H: the
// frame.  u of a pixel column px is (px + [0, 1)) / (W - 1), v of image row y
// is (H - 1 - y + [0, 1)) / (H - 1) (main.zig:390-391).
RTWB_HD Beam tile_beam(const double origin[3], const double llc[3], const double horizontal[3],
                       const double vertical[3], const double cu[3], const double cv[3], double lens_radius,
                       uint32_t W, uint32_t H, uint32_t px0, uint32_t px1, uint32_t y0, uint32_t y1) {
  const double w1 = (double)W - 1.0, h1 = (double)H - 1.0;
  const double s0 = (double)px0 / w1, s1 = ((double)px1 + 1.0) / w1;
  const double t0 = ((double)H - 1.0 - (double)y1) / h1, t1 = ((double)H - (double)y0) / h1;
  const double sc = 0.5 * (s0 + s1), tc = 0.5 * (t0 + t1), ds = 0.5 * (s1 - s0), dt = 0.5 * (t1 - t0);
  Beam b;
  double p2 = 0.0, m2 = 0.0, uu = 0.0, vv = 0.0, uv = 0.0;
  for (int k = 0; k < 3; ++k) {
    b.O[k] = origin[k];
    b.D[k] = (llc[k] + sc * horizontal[k] + tc * vertical[k]) - origin[k];
    const double p = ds * horizontal[k] + dt * vertical[k], m = ds * horizontal[k] - dt * vertical[k];
    p2 += p * p, m2 += m * m;
    uu += cu[k] * cu[k], vv += cv[k] * cv[k], uv += cu[k] * cv[k];
  }
  b.DD = b.D[0] * b.D[0] + b.D[1] * b.D[1] + b.D[2] * b.D[2];
  // |dx cu + dy cv|^2 <= largest eigenvalue of the Gram matrix <= max(uu, vv) + |uv| (Gershgorin)
  b.R = std::fabs(lens_radius) * std::sqrt(std::fmax(uu, vv) + std::fabs(uv));
  b.h = std::sqrt(std::fmax(p2, m2));  // a parallelogram's farthest points from its centre are corners
  // outward: the rounding of u, v and of the ray's own o, d (~1e-16 relative to these lengths)
  const double len = std::sqrt(b.DD) + std::sqrt(b.O[0] * b.O[0] + b.O[1] * b.O[1] + b.O[2] * b.O[2]);
  b.R = b.R * (1.0 + kRel) + kRel * len;
  b.h = b.h * (1.0 + kRel) + kRel * len;
  return b;
}

// min over l in [l0, l1] (l1 < 0: unbounded above) of g(l) <= its margin?
// qa > 0 is the caller's precondition (beam_may_hit's cone guard).
RTWB_HD bool beam_piece(const double E[3], const Beam& b, double alpha, double beta, double l0, double l1) {
  const double ED = E[0] * b.D[0] + E[1] * b.D[1] + E[2] * b.D[2];
  const double qa = b.DD - beta * beta, qb = ED - alpha * beta;
  double l = -qb / qa;  // the vertex
  l = std::fmax(l, l0);
  if (l1 >= 0.0) l = std::fmin(l, l1);
  const double x = E[0] + l * b.D[0], y = E[1] + l * b.D[1], z = E[2] + l * b.D[2];
  const double n2 = x * x + y * y + z * z, s = alpha + beta * l;
  const double scale = 2.0 * ((E[0] * E[0] + E[1] * E[1] + E[2] * E[2]) + l * l * b.DD) + s * s;
  return !(n2 - s * s > kRel * scale);  // (NaN: may be hit)
}

// The sphere's record: centre c0, travel dc = c1 - c0, radius (negative for a
// hollow shell), moving flag and its time group's [tg0, tg1] (centre(time) =
// c0 + dc (time - tg0) / (tg1 - tg0), hittable.zig:219-221); time0, time1: the
// camera's shutter.  false = no camera ray of the tile can hit it.
RTWB_HD bool beam_may_hit(const Beam& b, const double c0[3], const double dc[3], double radius, bool moving,
                          double tg0, double tg1, double time0, double time1) {
  double C[3] = {c0[0], c0[1], c0[2]};
  double r = std::fabs(radius);
  if (moving) {
    const double f0 = (time0 - tg0) / (tg1 - tg0), f1 = (time1 - tg0) / (tg1 - tg0);
    const double fm = 0.5 * (f0 + f1);
    const double fh = 0.5 * std::fabs(f1 - f0) * (1.0 + kRel) + kRel * (1.0 + std::fabs(fm));
    for (int k = 0; k < 3; ++k) C[k] = c0[k] + dc[k] * fm;
    r += fh * std::sqrt(dc[0] * dc[0] + dc[1] * dc[1] + dc[2] * dc[2]);
  }
  const double E[3] = {b.O[0] - C[0], b.O[1] - C[1], b.O[2] - C[2]};
  r = r * (1.0 + kRel) + kRel * std::sqrt(E[0] * E[0] + E[1] * E[1] + E[2] * E[2]);
  const double bw = b.h + b.R;
  if (!(b.DD - bw * bw > 1e-6 * (b.DD + bw * bw))) return true;  // cone wider than ~45 degrees (or NaN)
  // l in [0, 1]: rho = R + l (h - R);  l >= 1: rho = -R + l (h + R)
  if (beam_piece(E, b, r + b.R, b.h - b.R, 0.0, 1.0)) return true;
  return beam_piece(E, b, r - b.R, b.h + b.R, 1.0, -1.0);
}

}  // namespace rtwb
