// Host build of the product's Tier-B libm (csrc/rtw_libm.hpp) against the
// oracle's independent restatement (oracle/ro_libm.h) — must agree bit for
// bit — and against glibc (must be within 1 ulp).  Inputs: random doubles
// over many magnitudes, the exact multiples/cancellation points of pi/2 that
// select the argument-reduction branches, and special values
// (libm_inputs.hpp, shared with tests/native/gpu_contract_check.hip, which
// checks the gfx950 build), and that header's sphere-UV edges.
// Usage: libm_check N seed  -> "cases C mismatch M maxulp U"
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "libm_inputs.hpp"
#include "ro_libm.h"
#include "rtw_libm.hpp"

static int64_t ulps(double a, double b) {
  if (std::isnan(a) && std::isnan(b)) return 0;
  int64_t ia, ib;
  std::memcpy(&ia, &a, 8);
  std::memcpy(&ib, &b, 8);
  if ((ia < 0) != (ib < 0)) return a == b ? 0 : INT64_MAX;
  return ia > ib ? ia - ib : ib - ia;
}
static bool same(double a, double b) {
  uint64_t x, y;
  std::memcpy(&x, &a, 8);
  std::memcpy(&y, &b, 8);
  return x == y || (std::isnan(a) && std::isnan(b));
}

int main(int argc, char** argv) {
  // the generator lives in libm_inputs.hpp (shared with the device check), followed by the
  // sphere-UV edges and interval bounds that check adds
  std::vector<double> xs = libm_inputs(argc > 1 ? atol(argv[1]) : 1000000, argc > 2 ? atol(argv[2]) : 1);
  std::vector<double> ey, ex, ec;
  sphere_uv_edges(ey, ex, ec);
  long cases = 0, mismatch = 0;
  int64_t maxulp = 0;
  auto chk = [&](double a, double b, double ref) {
    ++cases;
    if (!same(a, b)) {
      if (mismatch < 5) printf("mismatch %.17g %.17g\n", a, b);
      ++mismatch;
    }
    const int64_t u = ulps(a, ref);
    if (u > maxulp) maxulp = u;
  };
  for (size_t i = 0; i < xs.size(); ++i) {
    const double x = xs[i];
    chk(rtwl::sin(x), ro_sin(x), std::sin(x));
    chk(rtwl::cos(x), ro_cos(x), std::cos(x));
    const double y = libm_atan2_partner(xs, i);
    chk(rtwl::atan2(y, x), ro_atan2(y, x), std::atan2(y, x));
    const double c = libm_acos_arg(x);
    chk(rtwl::acos(c), ro_acos(c), std::acos(c));
  }
  for (size_t i = 0; i < ey.size(); ++i) chk(rtwl::atan2(ey[i], ex[i]), ro_atan2(ey[i], ex[i]), std::atan2(ey[i], ex[i]));
  for (double c : ec) chk(rtwl::acos(c), ro_acos(c), std::acos(c));
  printf("cases %ld mismatch %ld maxulp %" PRId64 "\n", cases, mismatch, maxulp);
  return mismatch == 0 && maxulp <= 1 ? 0 : 1;
}
