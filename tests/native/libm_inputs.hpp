// Inputs of the Tier-B libm checks, shared by the host check
// (tests/native/libm_check.cpp: host builds of csrc/rtw_libm.hpp against
// oracle/ro_libm.h) and the device check (tests/native/gpu_contract_check.hip:
// the gfx950 build against the same oracle).
//   libm_inputs(n, seed): n random doubles over many magnitudes, the exact
//     multiples / cancellation points of pi/2 that select the argument-reduction
//     branches, and special values;
//   libm_atan2_partner / libm_acos_arg: how both checks derive atan2's second
//     argument and acos's argument from that list;
//   sphere_uv_edges(ys, xs, cs): the edges of Sphere.getSphereUv
//     (hittable.zig:145-150: atan2(-z, x), acos(-y) of unit-vector components)
//     and the neighbours of every interval bound of atan / atan2 / acos.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

inline std::vector<double> libm_inputs(long n, unsigned long seed) {
  std::mt19937_64 g(seed);
  std::uniform_real_distribution<double> U(-1.0, 1.0), E(-8.0, 6.5);
  std::vector<double> xs;
  for (long i = 0; i < n; ++i) xs.push_back(U(g) * std::pow(10.0, E(g)));
  const double pio2 = 1.57079632679489661923;
  for (int k = -64; k <= 64; ++k)  // branch points of __rem_pio2
    for (int d = -3; d <= 3; ++d) xs.push_back(std::nextafter(k * pio2, d < 0 ? -INFINITY : INFINITY) + d * 1e-16 * k);
  const double sp[] = {0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1e-300, -1e-300, 5e-324, INFINITY, -INFINITY, NAN,
                       0.4375, 1.1875, 2.4375, 0x1p66, 0x1p-27, 0x1p20 * pio2 * 0.999};
  for (double s : sp) xs.push_back(s);
  return xs;
}
inline double libm_atan2_partner(const std::vector<double>& xs, size_t i) { return xs[(i * 7919 + 13) % xs.size()]; }
inline double libm_acos_arg(double x) { return std::fmod(x, 1.0); }

// |x| >= 2^20 * pi/2: sin / cos leave the Tier-B definition (the platform's libm answers)
inline bool libm_payne_hanek(double x) {
  uint64_t u;
  std::memcpy(&u, &x, 8);
  const uint32_t ix = (uint32_t)(u >> 32) & 0x7fffffffu;
  return ix >= 0x413921fbu && ix < 0x7ff00000u;
}

// x and its `span` neighbours on each side (by bit pattern, both signs)
inline void libm_push_around(std::vector<double>& v, double x, int span = 3) {
  uint64_t u;
  std::memcpy(&u, &x, 8);
  for (int d = -span; d <= span; ++d) {
    const uint64_t w = u + (uint64_t)(int64_t)d;
    double y;
    std::memcpy(&y, &w, 8);
    v.push_back(y);
    v.push_back(-y);
  }
}

// atan2(ys[i], xs[i]) and acos(cs[j])
inline void sphere_uv_edges(std::vector<double>& ys, std::vector<double>& xs, std::vector<double>& cs) {
  auto pair = [&](double y, double x) {
    ys.push_back(y);
    xs.push_back(x);
  };
  std::vector<double> t;
  // x or z equal to +-0 (poles, the u seam and the quarter meridians)
  const double unit[] = {1.0, -1.0, 0.6, -0.6, 0x1p-30, -0x1p-30, 5e-324, -5e-324, 0.0, -0.0};
  for (double a : unit)
    for (double z : {0.0, -0.0}) {
      pair(z, a);
      pair(a, z);
    }
  // x == 1 exactly: atan2 returns atan(y) unchanged
  t.clear();
  for (double b : {0.0, 5e-324, 0x1p-1022, 0x1p-60, 0x1p-27, 0.25, 0.4375, 0.6875, 1.0, 1.1875, 2.4375, 0x1p66, 1e300})
    libm_push_around(t, b);
  for (double y : t) pair(y, 1.0);
  // the interval bounds of atan (|y/x| = 2^-27, 7/16, 11/16, 19/16, 39/16, 2^66), reached as an exact
  // quotient (x = +-2^k) in all four quadrants
  t.clear();
  for (double b : {0x1p-27, 0.4375, 0.6875, 1.1875, 2.4375, 0x1p66}) libm_push_around(t, b, 4);
  for (double r : t)
    for (double x : {2.0, -2.0, 0x1p-40, -0x1p-40, 0x1p300}) pair(r * x, x);  // (r * 2^k is exact)
  // |y/x| across atan2's 2^64 and 2^-64 cut-offs (it compares the exponent fields of the high words)
  t.clear();
  for (int e : {-66, -65, -64, -63, -62, 62, 63, 64, 65, 66}) libm_push_around(t, std::ldexp(1.0, e), 2);
  for (double r : t)
    for (double x : {1.5, -1.5, 0x1p-500, -0x1p-500}) pair(r * x, x);
  for (double r : t)
    for (double y : {1.75, -1.75}) pair(y, r);
  // unit vectors near the axes and the diagonals: x = cos(a), -z = sin(a) for a around k * pi/4
  for (int k = -4; k <= 4; ++k)
    for (int d = -20; d <= 20; ++d) {
      const double a = k * 0.78539816339744830962 + d * 0x1p-55 * (d % 3 ? 1.0 : 0x1p20);
      pair(std::sin(a), std::cos(a));
    }
  // infinities
  const double inf = INFINITY, with_inf[] = {inf, -inf, 1.0, -1.0, 0.0, -0.0};
  for (double a : {inf, -inf})
    for (double b : with_inf) {
      pair(a, b);
      pair(b, a);
    }
  // acos(-y): +-1 and the last values inside, |x| around 2^-57 (below: pi/2), around +-0.5 (the
  // switch between the polynomial and the sqrt forms), 0, and |x| > 1 (NaN)
  for (double b : {1.0, 0.5, 0x1p-57, 0x1p-56, 0.25, 0.75, 0x1p-1022, 0.999, 2.0}) libm_push_around(cs, b, 4);
  const double rest[] = {0.0, -0.0, 5e-324, -5e-324, inf, -inf, NAN};
  for (double b : rest) cs.push_back(b);
}
