// rtw_selfskip.hpp — the sphere a ray has just left: its exact test ended at the prefilter (f64 megakernel).
//
// A secondary ray starts on the sphere it was scattered from, so its LINE always meets that sphere and the
// packed-f32 pretest (rtw_cull.hpp) can never rule it out: the sphere gets the full exact test
// (Sphere.hit / MovingSphere.hit, hittable.zig:95-116, :165-186), which for a ray that leaves outwards can
// only end in "both roots below t_min".  Its cc = |oc|^2 - r^2 is a rounding error of either sign, so the
// older prefilter (cc > 0) let half of those tests go on to a square root and two divisions.
// `leaves` states a condition on the values the test computes FIRST — oc = o - centre(time), hb = oc.d (left
// to right), cc, a = |d|^2, all f64 — under which the test's remaining f64 arithmetic, as written in the
// reference, rejects the sphere.  It holds for ANY sphere with such values, not only the one just left, and
// closest_hit (rtw_device.hpp, LEAVEPRE) uses it as the prefilter of every exact test: on the test's own hb
// and cc, so no value of the rule can differ from the test's.
//
// Condition (u = 2^-53, every operation round-to-nearest):
//   2^-100 <= tmin <= 2^100,  2^-40 <= a <= 2^40,  2^-200 < hb < RN(2^50 tmin a),  cc > -RN(tmin hb).
// Proof (DESIGN.md §5.13 has it with every constant).  P = RN(hb^2), Q = RN(a cc), D = RN(P - Q).
//   cc >= 0: Q >= 0 and D <= P.  cc < 0: |Q| <= a tmin hb (1+u)^2 and D <= (P + |Q|)(1+u).  Either way
//   D <= (hb^2 + a tmin hb)(1+u)^3; no operand under- or overflows inside the ranges above.  D < 0 is a
//   reject.  Else sq = RN(sqrt D) <= (hb + a tmin / 2)(1+3u), as sqrt(h^2 + x) <= h + x / (2h).
//   root1 = RN(RN(-hb - sq) / a) <= 0 < tmin, so the test goes on to root2 = RN(RN(-hb + sq) / a).
//   sq <= hb gives root2 <= 0.  Else root2 <= [(a tmin / 2)(1+3u) + 3u hb](1+u)^2 / a
//   <= tmin (1/2 + 3u) + 3u 2^50 tmin (1+4u) = tmin (1/2 + 3/8 + 5u) < tmin: rejected.
// In exact arithmetic the condition bounds the second root by tmin / 2; the other half of tmin covers the
// rounding of hb^2 and of the square root, which the cancellation in -hb + sq turns into 3u hb / a — hence
// the upper limit on hb.  NaN operands fail a comparison and the rule does not fire; hb <= 0 (a ray that
// enters its sphere) does not either.  tests/native/selfskip_check.cpp states the reference's test literally
// and checks the rule against it on > 10^7 adversarial cases.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define RTWS_HD __host__ __device__ __forceinline__
#else
#define RTWS_HD inline
#endif

namespace rtws {

constexpr double kAMin = 0x1p-40, kAMax = 0x1p40;        // rtwc::lane_cull's range of |d|^2
constexpr double kTminMin = 0x1p-100, kTminMax = 0x1p100;
constexpr double kHbMin = 0x1p-200;                      // hb^2 and tmin * hb stay normal numbers
constexpr double kHbScale = 0x1p50;                      // hb < 2^50 tmin a: 3u hb / a <= (3/8) tmin
#ifndef RTW_SELFSKIP_CC_SCALE                            // (the checker's control builds loosen it)
#define RTW_SELFSKIP_CC_SCALE 1.0
#endif
constexpr double kCcScale = RTW_SELFSKIP_CC_SCALE;       // cc > -kCcScale * tmin * hb: exact root2 <= tmin / 2

// The upper limit of hb for a ray of |d|^2 = a: RN(2^50 tmin a), or 0 (no hb passes) outside the ranges.
RTWS_HD double hb_limit(double a, double tmin) {
  const bool range = (tmin >= kTminMin) & (tmin <= kTminMax) & (a >= kAMin) & (a <= kAMax);
  return range ? (tmin * kHbScale) * a : 0.0;
}
// The rule with that limit made once per ray (the closest hit's form: three compares and a product per sphere).
RTWS_HD bool leaves_lim(double hb, double cc, double tmin, double lim) {
  const double thr = (kCcScale == 1.0 ? tmin : tmin * kCcScale) * hb;
  return (hb > kHbMin) & (hb < lim) & (cc > -thr);
}
// True: the reference's f64 test of this sphere ends in a reject (disc < 0, or both roots below tmin).
RTWS_HD bool leaves(double hb, double cc, double a, double tmin) { return leaves_lim(hb, cc, tmin, hb_limit(a, tmin)); }

}  // namespace rtws
