// rtw_temporal.hpp — temporal accumulation (rtw_hip.h "temporal accumulation",
// DESIGN.md §18): where a pixel's surface point was in the previous frame,
// whether it was visible there, and the running mean and luminance moments of
// what was seen at it.  No HIP here: the kernels (rtw_temporal.hip), the host
// entries (rtw_temporal_host.cpp) and the native check
// (tests/native/temporal_check.cpp) compile the same functions, and the
// device's bytes equal the host's.
//
// Arithmetic: f64, one IEEE operation per operator (-ffp-contract=off), only
// + - * /, floor, fmin, fmax and comparisons; f32 inputs are widened (exact) and
// each output is rounded to f32 once, on store.  dot(a, b) = (a0 b0 + a1 b1) +
// a2 b2; cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).
//
// Per pixel (x, image row y), with the current mean c, the current guide g, the
// previous history image and the previous camera:
//  1. Where it was: (fx, fy) in the previous image, and the depth tp expected there.
//     * hit (g.prim != 0) with a previous point pp: q = pp - origin',
//       d0 = llc' - origin', n = cross(h', v') (d0, n: once per call, Proj); the
//       solution of d0 + s h' + t v' = mu q by Cramer's rule,
//         det = dot(q, n)   mu = dot(d0, n) / det
//         s = -dot(q, cross(d0, v')) / det   t = -dot(q, cross(h', d0)) / det;
//       invalid (no history) unless q, det, mu, s and t are finite, det != 0 and
//       mu > 0.  fx = s (W - 1) - 0.5, fy = ((H - 1) + 0.5) - t (H - 1) (the
//       inverse of the guides' s, t), tp = 1 / mu.  Snap: with r = floor(f + 0.5),
//       |f - r| <= 2^-10 makes f = r, for fx and fy each.
//     * hit without previous points (nothing moved): fx = x, fy = y, tp = g.depth.
//     * miss: fx = x, fy = y if the two cameras are bytewise equal, else no history.
//  2. Taps: (fx, fy) outside (-1, W) x (-1, H) has no history.  Else x0 =
//     floor(fx), wx = fx - x0 (y alike) and the four taps in row-major order are
//     (x0, y0): (1 - wx)(1 - wy), (x0 + 1, y0): wx (1 - wy), (x0, y0 + 1):
//     (1 - wx) wy, (x0 + 1, y0 + 1): wx wy.  A tap counts iff its weight is > 0,
//     it lies inside the image, its record has len > 0 and prim == g.prim, and,
//     for a hit, |rec.depth - tp| <= depth_tol * fmax(rec.depth, tp).  ws = the
//     counting weights summed in that order; ws < 2^-7: no history.
//  3. Blend, Y = luminance(c):
//     no history: {c, len 1, m1 = Y, m2 = Y Y}.
//     else hist = (sum w rec) / ws for mean, len, m1, m2 (each sum in tap order),
//     N = fmin(hist.len, max_history), a = 1 / (N + 1), and each of colour, m1,
//     m2 is hist + a (cur - hist); len = N + 1.  depth and prim: the guide's.
//  4. Variance out: fmax(0, m2 - m1 m1) / len when len >= min_len_var (the f64
//     values of step 3, before their rounding), else kVarUnknown.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rtw_denoise.hpp"
#include "rtw_world_refit.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTW_TP_HD __host__ __device__
#else
#define RTW_TP_HD
#endif

namespace rtwt {

using rtwd::Guide;

constexpr uint32_t kDefMaxHistory = 32, kMaxMaxHistory = 4096;
constexpr double kDefDepthTol = 0.02;
constexpr uint32_t kDefMinLenVar = 4;
constexpr double kSnap = 0x1p-10, kMinWeight = 0x1p-7;

struct alignas(16) History {  // = rtw_history
  float mean[3];
  float len;
  float m1, m2;
  float depth;
  uint32_t prim;
};
static_assert(sizeof(History) == 32, "two 16-byte loads");

struct Params {  // the resolved options of one call
  double max_history, depth_tol, min_len_var;
};

// 0 = default for every field; false: out of range.
RTW_TP_HD inline bool resolve(uint32_t max_history, double depth_tol, uint32_t min_len_var, uint32_t flags, Params& P) {
  if (flags != 0u || max_history > kMaxMaxHistory || min_len_var == 1u) return false;
  if (!(depth_tol >= 0.0 && depth_tol < 1e30)) return false;
  P.max_history = (double)(max_history ? max_history : kDefMaxHistory);
  P.depth_tol = depth_tol > 0.0 ? depth_tol : kDefDepthTol;
  P.min_len_var = (double)(min_len_var ? min_len_var : kDefMinLenVar);
  return true;
}

RTW_TP_HD inline bool finite(double x) { return x - x == 0.0; }
RTW_TP_HD inline double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
RTW_TP_HD inline void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// What the projection reads of the previous camera (made once per call, on the host).
struct Proj {
  double origin[3], h[3], v[3], d0[3], n[3];
};
RTW_TP_HD inline Proj make_proj(const double origin[3], const double horizontal[3], const double vertical[3],
                                const double llc[3]) {
  Proj c;
  for (int k = 0; k < 3; ++k) {
    c.origin[k] = origin[k], c.h[k] = horizontal[k], c.v[k] = vertical[k];
    c.d0[k] = llc[k] - origin[k];
  }
  cross3(c.h, c.v, c.n);
  return c;
}

RTW_TP_HD inline double snap(double f) {
  const double r = floor(f + 0.5), d = f - r;
  return (d <= kSnap && d >= -kSnap) ? r : f;
}

// Step 1 for a hit with a previous point: false = invalid.
RTW_TP_HD inline bool project(const Proj& c, double p0, double p1, double p2, int W, int H, double& fx, double& fy,
                              double& tp) {
  const double q[3] = {p0 - c.origin[0], p1 - c.origin[1], p2 - c.origin[2]};
  if (!(finite(q[0]) && finite(q[1]) && finite(q[2]))) return false;
  const double det = dot3(q, c.n);
  if (!finite(det) || det == 0.0) return false;
  double a[3], b[3];
  cross3(c.d0, c.v, a);
  cross3(c.h, c.d0, b);
  const double mu = dot3(c.d0, c.n) / det;
  const double s = -dot3(q, a) / det;
  const double t = -dot3(q, b) / det;
  if (!(finite(mu) && finite(s) && finite(t)) || !(mu > 0.0)) return false;
  fx = snap(s * (double)(W - 1) - 0.5);
  fy = snap(((double)(H - 1) + 0.5) - t * (double)(H - 1));
  tp = 1.0 / mu;
  return true;
}

struct Out {
  History rec;
  float var;
};

// One pixel.  hist(x, y) -> History reads an in-image record of the previous
// history (called only when has_hist).  (m0, m1c, m2c): the current mean; (p0, p1,
// p2): the previous point when has_pp.
template <typename HistAt>
RTW_TP_HD inline Out accumulate_pixel(int x, int y, int W, int H, const Params& P, float m0, float m1c, float m2c,
                                      const Guide& g, bool has_hist, bool has_pp, double p0, double p1, double p2,
                                      const Proj& cam_prev, bool same_cam, HistAt hist) {
  const double c0 = m0, c1 = m1c, c2 = m2c;
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
    o.rec.mean[0] = m0, o.rec.mean[1] = m1c, o.rec.mean[2] = m2c;
    len = 1.0, m1 = Y, m2 = Y * Y;
  } else {
    const double h0 = s0 / ws, h1 = s1 / ws, h2 = s2 / ws, hl = sl / ws, hm1 = sm1 / ws, hm2 = sm2 / ws;
    const double N = fmin(hl, P.max_history);
    const double a = 1.0 / (N + 1.0);
    o.rec.mean[0] = (float)(h0 + a * (c0 - h0));
    o.rec.mean[1] = (float)(h1 + a * (c1 - h1));
    o.rec.mean[2] = (float)(h2 + a * (c2 - h2));
    len = N + 1.0;
    m1 = hm1 + a * (Y - hm1);
    m2 = hm2 + a * (Y * Y - hm2);
  }
  o.rec.len = (float)len;
  o.rec.m1 = (float)m1;
  o.rec.m2 = (float)m2;
  o.rec.depth = g.depth;
  o.rec.prim = g.prim;
  o.var = len >= P.min_len_var ? (float)(fmax(0.0, m2 - m1 * m1) / len) : rtwd::kVarUnknown;
  return o;
}

// ---- the feature ray of a pixel (rtw_pixel_ray's expressions): 9 doubles = rtw_ray ----
RTW_TP_HD inline void pixel_ray(const double origin[3], const double horizontal[3], const double vertical[3],
                                const double llc[3], double time0, double time1, uint32_t W, uint32_t H, uint32_t x,
                                uint32_t y, double r[9]) {
  const double s = ((double)x + 0.5) / (double)(W - 1u);
  const double t = ((double)(H - 1u - y) + 0.5) / (double)(H - 1u);
  for (int k = 0; k < 3; ++k) {
    r[k] = origin[k];
    r[3 + k] = ((llc[k] + horizontal[k] * s) + vertical[k] * t) - origin[k];
  }
  r[6] = time0 + 0.5 * (time1 - time0);
  r[7] = 0.001;
  r[8] = __builtin_huge_val();
}

// ---- where a hit's surface point was under other numbers ----
// p, nrm, u, v, front: the hit record's (of the world as it is now).  kind:
// rtw_prim_kind.  r_prev: doubles 0-8 of the primitive's record under the
// PREVIOUS numbers (rtwr::fill_record).  xf_h: the header word of its transform
// chain (0: none); v_now / v_prev: the chain's values, three per op, now and
// before.  The surface parameters come from the record alone: the outward
// object-space normal (the record's, negated when front == 0, taken back through
// the current chain as a direction: RotateY's to_object, Translate does nothing)
// for a sphere, (u, v) for a rect.  moved == false (both arrays NULL): p itself.
RTW_TP_HD inline void prev_point(const double p[3], const double nrm[3], double u, double v, uint32_t front,
                                 uint32_t kind, const double r_prev[9], uint32_t xf_h, const double* v_now,
                                 const double* v_prev, double time, bool moved, double out[3]) {
  if (!moved) {
    out[0] = p[0], out[1] = p[1], out[2] = p[2];
    return;
  }
  const int n = (int)rtwr::xform_ops(xf_h);
  double q0, q1, q2;
  if (kind <= 1u) {
    double n0 = front ? nrm[0] : -nrm[0], n1 = front ? nrm[1] : -nrm[1], n2 = front ? nrm[2] : -nrm[2];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < (int)rtwk::kMaxXfOps; ++i) {
      if (i >= n) break;
      if (rtwr::xform_op(xf_h, i) != 0u) {
        const double sn = v_now[3 * i], cs = v_now[3 * i + 1];
        const double a = n0, b = n2;
        n0 = cs * a - sn * b;
        n2 = sn * a + cs * b;
      }
    }
    double c0 = r_prev[0], c1 = r_prev[1], c2 = r_prev[2];
    if (kind == 1u) {
      const double f = (time - r_prev[7]) / r_prev[8];
      c0 = c0 + r_prev[3] * f, c1 = c1 + r_prev[4] * f, c2 = c2 + r_prev[5] * f;
    }
    q0 = c0 + r_prev[6] * n0, q1 = c1 + r_prev[6] * n1, q2 = c2 + r_prev[6] * n2;
  } else {
    const double a = r_prev[0] + u * r_prev[5], b = r_prev[2] + v * r_prev[6], k = r_prev[4];
    if (kind == 2u) q0 = a, q1 = b, q2 = k;
    else if (kind == 3u) q0 = a, q1 = k, q2 = b;
    else q0 = k, q1 = a, q2 = b;
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = (int)rtwk::kMaxXfOps - 1; i >= 0; --i) {
    if (i >= n) continue;
    const double w0 = v_prev[3 * i], w1 = v_prev[3 * i + 1], w2 = v_prev[3 * i + 2];
    if (rtwr::xform_op(xf_h, i) == 0u) {
      q0 = q0 + w0, q1 = q1 + w1, q2 = q2 + w2;
    } else {
      const double a = q0, b = q2;
      q0 = w1 * a + w0 * b;
      q2 = -w0 * a + w1 * b;
    }
  }
  out[0] = q0, out[1] = q1, out[2] = q2;
}

// ---- library internals (rtw_temporal_host.cpp), shared by the host and device entries ----
int check_call(const char* who, const void* mean, const void* guides, const void* prev_p, const void* cam_prev,
               const void* cam, const void* hist_in, uint32_t W, uint32_t H, uint32_t max_history, double depth_tol,
               uint32_t min_len_var, uint32_t flags, const void* hist_out, const void* mean_out, const void* var_out,
               Params& P);

}  // namespace rtwt
