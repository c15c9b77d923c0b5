// rtw_temporal_clamp.hpp — temporal accumulation with the history clamped to the
// current frame's neighbourhood (rtw_hip.h rtw_temporal_clamped_*).
// No HIP here: the kernel (rtw_temporal_clamp.hip), the host entry
// (rtw_temporal_clamp_host.cpp) and the native check
// (tests/native/temporal_clamp_check.cpp) compile the same function, and the
// device's bytes equal the host's.
//
// Arithmetic: rtw_temporal.hpp's rules (f64, one IEEE operation per operator,
// f32 inputs widened, each output rounded to f32 once) with sqrt in addition
// (correctly rounded on both sides, as rtw_denoise.hpp relies on).
//
// Per pixel, steps 1 and 2 of rtw_temporal.hpp unchanged (where it was, the four
// taps, ws, the no-history case).  With history, between hist = the
// weight-normalised taps and the blend:
//  a. Window: the pixels (x + dx, y + dy), |dx|, |dy| <= r, dy outer, dx inner.
//     cur(qx, qy) gives a window pixel's current mean and NaN channels for a
//     position outside the image; a pixel with a channel c where c - c != 0 is
//     skipped, so the image's border and a bad pixel are one rule.  Over the n
//     counted pixels, per channel: s = sum c, s2 = sum c c, mu = s / n,
//     var = fmax(0, s2 / n - mu mu), sg = sqrt(var), lo = mu - gamma sg,
//     hi = mu + gamma sg.
//  b. n < 4: the history is left alone.  Else h' = fmin(fmax(h, lo), hi) per channel.
//  c. No channel changed: nothing else does (bytewise the unclamped path).  Else
//     d = luminance(h') - luminance(h), hm2' = (hm2 + (2 hm1) d) + d d,
//     hm1' = hm1 + d: the accumulated luminance distribution moves to the clamped
//     mean and keeps its variance.  len is untouched.
//  Steps 3 and 4 of rtw_temporal.hpp then run on h', hm1', hm2'.
//  A bad pixel of the current mean leaves a non-finite record behind, and the next
//  frame computes with it (the clamp brings such a history's colour back into the
//  window's range; its moments become NaN until the blend has forgotten them).
//  Which NaN an operation returns, its sign and payload, is the instruction set's
//  business: x86 and gfx950 differ in inf - inf alone.  So every value this
//  function computes is stored through store_f32, which writes the one quiet NaN
//  0x7FC00000 for any NaN; a first frame's mean is the input's bytes as before.
#pragma once
#include "rtw_temporal.hpp"

namespace rtwt {

constexpr double kDefClampGamma = 0.5;  // the rule that chose it
constexpr uint32_t kDefClampRadius = 1, kMaxClampRadius = 3;
constexpr int kClampMinCount = 4;

struct Clamp {  // the resolved rtw_temporal_clamp of one call
  double gamma;
  int radius;
};

// 0 = default for every field; false: out of range.
RTW_TP_HD inline bool resolve_clamp(double gamma, uint32_t radius, uint32_t reserved, Clamp& K) {
  if (reserved != 0u || radius > kMaxClampRadius) return false;
  if (!(gamma >= 0.0 && gamma < 1e30)) return false;
  K.gamma = gamma > 0.0 ? gamma : kDefClampGamma;
  K.radius = (int)(radius ? radius : kDefClampRadius);
  return true;
}

RTW_TP_HD inline float store_f32(double v) { return v == v ? (float)v : __builtin_nanf(""); }

struct Rgb {
  float c0, c1, c2;
};

// One pixel.  hist(qx, qy) -> History as in accumulate_pixel (in-image positions
// only); cur(qx, qy) -> Rgb for every position of the pixel's window, NaN outside
// the image.  The pixel's own mean is cur(x, y).
template <typename HistAt, typename CurAt>
RTW_TP_HD inline Out accumulate_pixel_clamped(int x, int y, int W, int H, const Params& P, double gamma, int radius,
                                              const Guide& g, bool has_hist, bool has_pp, double p0, double p1,
                                              double p2, const Proj& cam_prev, bool same_cam, HistAt hist, CurAt cur) {
  const Rgb m = cur(x, y);
  const double c0 = m.c0, c1 = m.c1, c2 = m.c2;
  const double Y = rtwd::luminance(c0, c1, c2);
  const bool is_hit = g.prim != 0u;
  double fx = (double)x, fy = (double)y, tp = (double)g.depth;
  bool valid = has_hist;
  if (valid) {
    if (is_hit) {
      if (has_pp) valid = project(cam_prev, p0, p1, p2, W, H, fx, fy, tp);
    } else {
      valid = same_cam;
    }
  }
  double ws = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, sl = 0.0, sm1 = 0.0, sm2 = 0.0;
  if (valid && fx > -1.0 && fx < (double)W && fy > -1.0 && fy < (double)H) {
    const double bx = floor(fx), by = floor(fy);
    const double wx = fx - bx, wy = fy - by;
    const int x0 = (int)bx, y0 = (int)by;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
      const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
      const double w = ((k & 1) ? wx : 1.0 - wx) * ((k >> 1) ? wy : 1.0 - wy);
      if (!(w > 0.0) || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
      const History r = hist(qx, qy);
      if (!(r.len > 0.0f) || r.prim != g.prim) continue;
      if (is_hit) {
        const double rd = r.depth, d = rd - tp;
        if (!(fmax(d, -d) <= P.depth_tol * fmax(rd, tp))) continue;
      }
      ws += w;
      s0 += w * (double)r.mean[0];
      s1 += w * (double)r.mean[1];
      s2 += w * (double)r.mean[2];
      sl += w * (double)r.len;
      sm1 += w * (double)r.m1;
      sm2 += w * (double)r.m2;
    }
  }
  Out o;
  double len, m1, m2;
  if (ws < kMinWeight) {
    o.rec.mean[0] = m.c0, o.rec.mean[1] = m.c1, o.rec.mean[2] = m.c2;
    len = 1.0, m1 = Y, m2 = Y * Y;
  } else {
    double h0 = s0 / ws, h1 = s1 / ws, h2 = s2 / ws, hm1 = sm1 / ws, hm2 = sm2 / ws;
    const double hl = sl / ws;
    // a. the window's statistics
    double n = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0;
    for (int dy = -radius; dy <= radius; ++dy)
      for (int dx = -radius; dx <= radius; ++dx) {
        const Rgb v = cur(x + dx, y + dy);
        const double v0 = v.c0, v1 = v.c1, v2 = v.c2;
        if (!(finite(v0) && finite(v1) && finite(v2))) continue;
        n += 1.0;
        a0 += v0, a1 += v1, a2 += v2;
        q0 += v0 * v0, q1 += v1 * v1, q2 += v2 * v2;
      }
    if (n >= (double)kClampMinCount) {
      // b. the clamp
      const double mu0 = a0 / n, mu1 = a1 / n, mu2 = a2 / n;
      const double g0 = gamma * sqrt(fmax(0.0, q0 / n - mu0 * mu0));
      const double g1 = gamma * sqrt(fmax(0.0, q1 / n - mu1 * mu1));
      const double g2 = gamma * sqrt(fmax(0.0, q2 / n - mu2 * mu2));
      const double k0 = fmin(fmax(h0, mu0 - g0), mu0 + g0);
      const double k1 = fmin(fmax(h1, mu1 - g1), mu1 + g1);
      const double k2 = fmin(fmax(h2, mu2 - g2), mu2 + g2);
      if (!(k0 == h0 && k1 == h1 && k2 == h2)) {
        // c. the moments follow the mean
        const double d = rtwd::luminance(k0, k1, k2) - rtwd::luminance(h0, h1, h2);
        hm2 = (hm2 + (2.0 * hm1) * d) + d * d;
        hm1 = hm1 + d;
        h0 = k0, h1 = k1, h2 = k2;
      }
    }
    const double N = fmin(hl, P.max_history);
    const double a = 1.0 / (N + 1.0);
    o.rec.mean[0] = store_f32(h0 + a * (c0 - h0));
    o.rec.mean[1] = store_f32(h1 + a * (c1 - h1));
    o.rec.mean[2] = store_f32(h2 + a * (c2 - h2));
    len = N + 1.0;
    m1 = hm1 + a * (Y - hm1);
    m2 = hm2 + a * (Y * Y - hm2);
  }
  o.rec.len = (float)len;
  o.rec.m1 = store_f32(m1);
  o.rec.m2 = store_f32(m2);
  o.rec.depth = g.depth;
  o.rec.prim = g.prim;
  o.var = len >= P.min_len_var ? (float)(fmax(0.0, m2 - m1 * m1) / len) : rtwd::kVarUnknown;
  return o;
}

// ---- library internals (rtw_temporal_clamp_host.cpp), shared by the host and device entries ----
int check_clamp(const char* who, double gamma, uint32_t radius, uint32_t reserved, Clamp& K);

}  // namespace rtwt
