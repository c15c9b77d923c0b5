// rtw_denoise.hpp — the feature-guided denoiser's filter (rtw_hip.h
// rtw_denoise_*).  No HIP here: the device kernels
// (rtw_denoise.hip), the host restatement (rtw_denoise_host.cpp) and the native
// check (tests/native/denoise_check.cpp) compile the same function, and the
// device's bytes equal the host's.
//
// An edge-avoiding a-trous wavelet filter: `levels` iterations over the image,
// iteration l with the 5x5 B3-spline taps (1/16, 1/4, 3/8, 1/4, 1/16 per axis)
// spaced 2^l pixels apart.  An image pixel is {r, g, b, var}: the linear colour
// and the variance of its luminance estimate, Y = (0.2126 r + 0.7152 g) +
// 0.0722 b.  var >= 0: known; var < 0: unknown (kVarUnknown = -1); var <=
// kVarEmptyBelow (kVarEmpty = -2): the pixel holds no sample at all.
//
// The weight of tap q for the centre p is  w = h * wn * (N / D)^2  with
//   h   the spline weight of the tap (a product of two powers of two and threes: exact),
//   wn  = tn * tn,  tn = fmax(0, 1 - (1 - fmin(dot(n_p, n_q), 1)) / sigma_normal)
//         (a cone around the centre's normal: 0 once 1 - dot reaches sigma_normal),
//   N   = c2 * z2 * a2        D = (c2 + dY^2) * (z2 + dz^2) * (a2 + da2)
//   c2  = (sigma_color * sqrt(var_p) + kEpsColor)^2,  dY = Y_p - Y_q          (colour; at the first level
//         var_p is here the 3x3 binomial mean (1/4, 1/2, 1/4 per axis) of the known variances around p:
//         a variance estimated from a few chunks is itself noisy)
//   z2  = (sigma_depth * fmax(depth_p, depth_q))^2,   dz = depth_p - depth_q  (depth, relative to the depths)
//   a2  = sigma_albedo^2,                             da2 = |albedo_p - albedo_q|^2
// i.e. each of the colour, depth and albedo terms is the rational bell
// (s^2 / (s^2 + d^2))^2 — 1 at d = 0, 1/4 at d = s, ~ (s/d)^4 beyond — and the
// three share ONE division per tap.  No exp, no libm beyond sqrt / fmin / fmax.
//   * var_p unknown, or kFlagNoColor: the colour term is dropped (c2 and its
//     factor of D are both 1), by the same code path — so unknown variance
//     gives the bytes of the colour term switched off.
//   * no guides: wn, the depth and the albedo terms are dropped the same way.
//   * p a miss (prim == 0) and q a hit, or the reverse: the tap is dropped (a
//     hard stop).  Two misses: the guide terms are 1 (nothing to compare).
//   * q outside the image, or empty: the tap is dropped.  p empty: the pixel
//     stays {0, 0, 0, var_p}.
// Output: colour' = sum(w c_q) / sum(w), var' = sum(w^2 var_q) / sum(w)^2 where
// var_p is known (an unknown var_q counts as var_p), else var' = var_p; the
// sums run over the 25 taps in row-major order (dy = -2..2 outer, dx = -2..2
// inner).  sum(w) = 0 (a degenerate normal) leaves the pixel as it is.
//
// Arithmetic: the f32 inputs are widened to f64 (exact), every operation below
// is one IEEE f64 operation per operator (-ffp-contract=off) — f64 division
// and square root are correctly rounded on the device as on the host, so no
// f32 operation's rounding mode, denormal handling or division expansion is
// part of the contract — and each result is rounded to f32 once, on store.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTW_DN_HD __host__ __device__
#else
#define RTW_DN_HD
#endif

namespace rtwd {

constexpr uint32_t kMaxLevels = 6, kDefaultLevels = 5;
// Defaults (rtw_denoise_opts fields left 0).  sigma_color 2: a tap two standard
// errors of the centre's luminance away keeps 1/4 of its weight; sigma_normal
// 0.1: the cone closes at ~26 degrees; sigma_depth 0.25: a tap a quarter of the
// depth away keeps 1/4; sigma_albedo 0.1 per unit colour.  Chosen on the
// oracle's 80-spp frames of the cover scene and the Cornell box (DESIGN.md
// §14.5: the error against a 1000-spp frame is flat within 2 % for sigma_color
// 1.5-2.5, and rises past the input's at 4).
constexpr double kDefSigmaColor = 2.0, kDefSigmaNormal = 0.1, kDefSigmaDepth = 0.25, kDefSigmaAlbedo = 0.1;
constexpr double kEpsColor = 1e-3;  // luminance units: the floor of the colour scale at var = 0
constexpr uint32_t kFlagNoColor = 1u;  // rtw_denoise_opts.flags bit 0: drop the colour term everywhere
constexpr uint32_t kFlagDirect = 2u;   // bit 1: the device runs every level in its direct form (same bytes; for A/B)
constexpr uint32_t kFlagSpatialVar = 4u;  // bit 2: unknown variances are estimated from the image first (below)
constexpr uint32_t kFlagsKnown = 7u;
constexpr float kVarUnknown = -1.0f, kVarEmpty = -2.0f, kVarEmptyBelow = -1.5f;

struct alignas(16) Px {  // an image pixel of the ping-pong buffers
  float r, g, b, var;
};
struct alignas(16) Guide {  // = rtw_guide
  float n[3];
  float depth;
  float albedo[3];
  uint32_t prim;
};
static_assert(sizeof(Px) == 16 && sizeof(Guide) == 32, "16-byte records");

struct Params {  // the resolved options of one call
  uint32_t levels, flags;
  double sigma_color, inv_sigma_normal, sigma_depth, a2;
};

// 0 = default for every field; false: out of range (levels > kMaxLevels, a
// negative or non-finite sigma, an unknown flag).
RTW_DN_HD inline bool resolve(uint32_t levels, double sc, double sn, double sd, double sa, uint32_t flags, Params& P) {
  if (levels > kMaxLevels || (flags & ~kFlagsKnown)) return false;
  const double big = 1e30;
  if (!(sc >= 0.0 && sc < big) || !(sn >= 0.0 && sn < big) || !(sd >= 0.0 && sd < big) || !(sa >= 0.0 && sa < big))
    return false;
  P.levels = levels ? levels : kDefaultLevels;
  P.flags = flags;
  P.sigma_color = sc > 0.0 ? sc : kDefSigmaColor;
  P.inv_sigma_normal = 1.0 / (sn > 0.0 ? sn : kDefSigmaNormal);
  P.sigma_depth = sd > 0.0 ? sd : kDefSigmaDepth;
  const double a = sa > 0.0 ? sa : kDefSigmaAlbedo;
  P.a2 = a * a;
  return true;
}

RTW_DN_HD inline double spline_tap(int i) {  // i = -2..2
  return i == 0 ? 0.375 : (i == 1 || i == -1) ? 0.25 : 0.0625;
}

RTW_DN_HD inline double luminance(double r, double g, double b) { return (0.2126 * r + 0.7152 * g) + 0.0722 * b; }

// finalize_kernel's quantisation (rtw_trace.hip; main.zig:395-400) of a mean value.
RTW_DN_HD inline uint8_t quantise(double mean) {
  const double g = sqrt(mean);
  const double cl = fmax(0.0, fmin(g, 0.999));
  return (uint8_t)(256.0 * cl);
}

// One pixel of one level.  px(x, y) -> Px and gd(x, y) -> Guide read an
// in-image pixel (gd is called only when GUIDES); `step` is the tap spacing.
template <bool GUIDES, typename PxAt, typename GuideAt>
RTW_DN_HD inline Px filter_pixel(int x, int y, int W, int H, int step, const Params& P, PxAt px, GuideAt gd) {
  const Px cp = px(x, y);
  if (cp.var <= kVarEmptyBelow) return Px{0.0f, 0.0f, 0.0f, cp.var};
  const double rp = cp.r, gp = cp.g, bp = cp.b, vp = cp.var;
  const double yp = luminance(rp, gp, bp);
  const bool known = vp >= 0.0;
  const bool colour = known && !(P.flags & kFlagNoColor);
  double c2 = 1.0;
  if (colour) {
    double v = vp;
    if (step == 1) {  // the first level: the 3x3 prefilter of the raw estimate
      double sv3 = 0.0, sk3 = 0.0;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int qx = x + dx, qy = y + dy;
          if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
          const double vq = px(qx, qy).var;
          if (!(vq >= 0.0)) continue;
          const double k = (dy == 0 ? 0.5 : 0.25) * (dx == 0 ? 0.5 : 0.25);
          sv3 += k * vq;
          sk3 += k;
        }
      v = sv3 / sk3;  // (sk3 >= 1/4: the centre is known)
    }
    const double s = P.sigma_color * sqrt(v) + kEpsColor;
    c2 = s * s;
  }
  Guide g0{};
  bool miss_p = false;
  if (GUIDES) {
    g0 = gd(x, y);
    miss_p = g0.prim == 0u;
  }
  double sw = 0.0, sr = 0.0, sg = 0.0, sb = 0.0, sv = 0.0;
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = y + dy * step;
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = x + dx * step;
      if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
      const Px cq = px(qx, qy);
      if (cq.var <= kVarEmptyBelow) continue;
      const double rq = cq.r, gq = cq.g, bq = cq.b;
      double wn = 1.0, num = c2, den = 1.0;
      if (colour) {
        const double dY = yp - luminance(rq, gq, bq);
        den = c2 + dY * dY;
      }
      if (GUIDES) {
        const Guide g1 = gd(qx, qy);
        if ((g1.prim == 0u) != miss_p) continue;
        if (!miss_p) {
          const double dn = ((double)g0.n[0] * (double)g1.n[0] + (double)g0.n[1] * (double)g1.n[1]) +
                            (double)g0.n[2] * (double)g1.n[2];
          const double tn = fmax(0.0, 1.0 - (1.0 - fmin(dn, 1.0)) * P.inv_sigma_normal);
          wn = tn * tn;
          const double zp = g0.depth, zq = g1.depth;
          const double mz = P.sigma_depth * fmax(zp, zq);
          const double z2 = mz * mz;
          const double dz = zp - zq;
          const double a0 = (double)g0.albedo[0] - (double)g1.albedo[0];
          const double a1 = (double)g0.albedo[1] - (double)g1.albedo[1];
          const double a2 = (double)g0.albedo[2] - (double)g1.albedo[2];
          const double da2 = (a0 * a0 + a1 * a1) + a2 * a2;
          num = (num * z2) * P.a2;
          den = (den * (z2 + dz * dz)) * (P.a2 + da2);
        }
      }
      const double q = num / den;
      const double w = (spline_tap(dy) * spline_tap(dx)) * wn * (q * q);
      if (!(w > 0.0)) continue;  // (also a NaN from a degenerate guide: 0 / 0)
      sw += w;
      sr += w * rq;
      sg += w * gq;
      sb += w * bq;
      const double vq = cq.var;
      sv += (w * w) * (vq >= 0.0 ? vq : vp);
    }
  }
  if (!(sw > 0.0)) return cp;
  Px o;
  o.r = (float)(sr / sw);
  o.g = (float)(sg / sw);
  o.b = (float)(sb / sw);
  o.var = known ? (float)(sv / (sw * sw)) : cp.var;
  return o;
}

// ---- the spatial variance estimate (kFlagSpatialVar) ----
// A pixel whose variance is unknown — fewer than two chunks in the accumulator
// — gets the guide-weighted variance of the luminance of the image itself over
// its 7x7 window (SVGF's fallback for a pixel without history):
//   var = fmax(0, s2 / sw - (s1 / sw)^2),  sw = sum w, s1 = sum w Y_q, s2 = sum w Y_q^2
// over the 49 taps in row-major order (dy = -3..3 outer, dx inner), the centre
// included.  w is filter_pixel's weight with the spline and colour terms left
// out, the same expressions in the same order: w = wn * q^2, q = (z2 * a2) /
// ((z2 + dz^2) * (a2 + da2)); two misses, or no guides: w = 1.  Dropped: a tap
// outside the image, an empty tap, a tap across the hit / miss border, a tap
// with !(w > 0).  Fewer than kSpatialMinTaps kept taps: the pixel stays
// unknown.  A known or an empty centre keeps its value bit for bit.  The mean
// image holds a pixel's mean already, so the window variance is in the units of
// the accumulator's squared standard error and feeds c2 as it is.  No bias
// correction (measured: never better).  Arithmetic as above: f64, one
// operation per operator, rounded to f32 once.
constexpr int kSpatialRadius = 3;
constexpr int kSpatialMinTaps = 4;

struct SvTap {  // what the estimate reads of a tap's pixel
  double y;     // luminance of its mean
  bool empty;
};
RTW_DN_HD inline SvTap sv_tap(const Px& p) {
  return SvTap{luminance((double)p.r, (double)p.g, (double)p.b), p.var <= kVarEmptyBelow};
}

// The new variance of pixel (x, y), whose variance is var_p.  tap(x, y) ->
// SvTap and gd(x, y) -> Guide read an in-image pixel (gd only when GUIDES).
template <bool GUIDES, typename TapAt, typename GuideAt>
RTW_DN_HD inline float spatial_variance_pixel(int x, int y, int W, int H, const Params& P, float var_p, TapAt tap,
                                              GuideAt gd) {
  if (var_p <= kVarEmptyBelow || var_p >= 0.0f) return var_p;
  Guide g0{};
  bool miss_p = false;
  if (GUIDES) {
    g0 = gd(x, y);
    miss_p = g0.prim == 0u;
  }
  double sw = 0.0, s1 = 0.0, s2 = 0.0;
  int kept = 0;
  for (int dy = -kSpatialRadius; dy <= kSpatialRadius; ++dy) {
    const int qy = y + dy;
    for (int dx = -kSpatialRadius; dx <= kSpatialRadius; ++dx) {
      const int qx = x + dx;
      if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
      const SvTap t = tap(qx, qy);
      if (t.empty) continue;
      double w = 1.0;
      if (GUIDES) {
        const Guide g1 = gd(qx, qy);
        if ((g1.prim == 0u) != miss_p) continue;
        if (!miss_p) {
          const double dn = ((double)g0.n[0] * (double)g1.n[0] + (double)g0.n[1] * (double)g1.n[1]) +
                            (double)g0.n[2] * (double)g1.n[2];
          const double tn = fmax(0.0, 1.0 - (1.0 - fmin(dn, 1.0)) * P.inv_sigma_normal);
          const double wn = tn * tn;
          const double zp = g0.depth, zq = g1.depth;
          const double mz = P.sigma_depth * fmax(zp, zq);
          const double z2 = mz * mz;
          const double dz = zp - zq;
          const double a0 = (double)g0.albedo[0] - (double)g1.albedo[0];
          const double a1 = (double)g0.albedo[1] - (double)g1.albedo[1];
          const double a2 = (double)g0.albedo[2] - (double)g1.albedo[2];
          const double da2 = (a0 * a0 + a1 * a1) + a2 * a2;
          const double q = (z2 * P.a2) / ((z2 + dz * dz) * (P.a2 + da2));
          w = wn * (q * q);
        }
      }
      if (!(w > 0.0)) continue;  // (also a NaN from a degenerate guide: 0 / 0)
      sw += w;
      s1 += w * t.y;
      s2 += w * (t.y * t.y);
      ++kept;
    }
  }
  if (kept < kSpatialMinTaps) return kVarUnknown;
  const double m1 = s1 / sw;
  return (float)fmax(0.0, s2 / sw - m1 * m1);
}

// ---- library internals (rtw_denoise_host.cpp), shared by the host and device entries ----
// Two ping-pong images of Px, each rounded up to 256 bytes.
inline size_t image_bytes(uint32_t W, uint32_t H) { return (((size_t)W * H * sizeof(Px)) + 255) & ~(size_t)255; }
// The argument check of rtw_denoise_device / rtw_denoise_host: RTW_OK and the
// resolved options, or RTW_EINVAL with the message set.
int check_call(const char* who, const void* mean, uint32_t W, uint32_t H, uint32_t levels, double sc, double sn,
               double sd, double sa, uint32_t flags, const void* workspace, size_t workspace_bytes, const void* rgb_out,
               const void* mean_out, Params& P);
// The same for rtw_denoise_spatial_variance_device / _host.
int check_spatial_call(const char* who, const void* mean, const void* var_in, const void* guides, uint32_t W, uint32_t H,
                       uint32_t levels, double sc, double sn, double sd, double sa, uint32_t flags, const void* var_out,
                       Params& P);
// The estimate over host buffers: var_out[i] for every pixel (var_in NULL: all unknown).
void spatial_variance_image(const float* mean, const float* var_in, const Guide* guides, uint32_t W, uint32_t H,
                            const Params& P, float* var_out);

}  // namespace rtwd
