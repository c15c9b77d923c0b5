// rtw_specular.hpp — where a mirror showed the same reflected thing in the
// previous frame (rtw_hip.h "mirror points").  No HIP here: the
// kernels (rtw_specular.hip), the host entries (rtw_specular_host.cpp) and the
// native check (tests/native/specular_check.cpp) compile the same functions, and
// the device's bytes equal the host's.
//
// Arithmetic: f64, one IEEE operation per operator (-ffp-contract=off), only
// + - * /, sqrt, fmin, fmax and comparisons; finite(x) is x - x == 0.
// dot(a, b) = (a0 b0 + a1 b1) + a2 b2; cross(a, b) = (a1 b2 - a2 b1, a2 b0 -
// a0 b2, a0 b1 - a1 b0); len(a) = sqrt(dot(a, a)); unit(a) = a / len(a), three
// divisions; a + s b is a_k + s * b_k per component.
//
// Reflected ray of a record (ray r, hit h): origin h.p, direction
// d - k n with k = 2 * dot(d, n), d the ray's unnormalised direction, n the
// record's normal; the ray's time, t_min 0.001, t_max +inf.
//
// prev_normal: the record's normal through the current chain as a direction
// (ops 0..n-1, RotateY: (cs a - sn b, sn a + cs b) on (x, z) with the current
// sin, cos; Translate nothing), then forward through the previous values (ops
// n-1..0, RotateY: (w1 a + w0 b, -w0 a + w1 b)): prev_point's two loops.
// moved == false: the record's normal itself.
//
// mirror_point (Mg, ng, O, target) -> M.  The target is a point S (tsky == false)
// or a unit direction r (the sky).  In this order:
//  0. Every input finite, else Mg.  vo = O - Mg, lo = len(vo), cos = dot(vo / lo, ng);
//     cos > 0 and finite, else Mg.
//  1. Rect (kind >= 2): point target: h = dot(S - Mg, ng), h > 0 else Mg, P = S -
//     (2 h) ng, dir = P - O; sky: h = dot(r, ng), h > 0 else Mg, dir = r - (2 h) ng.
//     den = dot(dir, ng); den == 0 or not finite: Mg.  s = dot(Mg - O, ng) / den;
//     M = O + s dir; not finite: Mg.
//  2. Sphere (kind <= 1), radius rp > 0 else Mg, c = Mg - rp ng.
//     Predictor: kappa = (1 / cos + cos) / rp, finite else Mg.  Point target: vs = S -
//     Mg, ds = len(vs), q = 1 + ds kappa, q > 0 and finite else Mg, h = dot(vs, ng),
//     V = Mg + (vs - (2 h) ng) / q.  Sky: h = dot(r, ng), V = Mg + (r - (2 h) ng) /
//     kappa.  Ray O -> V against the sphere: dv = V - O, oc = O - c, a = dot(dv, dv),
//     hb = dot(oc, dv), cc = dot(oc, oc) - rp rp, disc = hb hb - a cc; with disc >= 0,
//     a > 0, t = (-hb - sqrt(disc)) / a > 0 and the result finite: n0 = unit((oc + t
//     dv)), else n0 = ng.
//     Newton, `steps` times, on f(n) = |M - O| + |M - S| over M = c + rp n:
//     state(n): M = c + rp n, va = M - O, la = len(va), a = va / la, ila = 1 / la;
//     point: vb = M - S, lb = len(vb), b = vb / lb, ilb = 1 / lb; sky: b = -r, ilb =
//     0.  w = a + b (made again where it is read), wn = dot(w, n), tang = w - wn n,
//     T = dot(tang, tang).
//     step: ax = (n.x n.x > 0.5) ? y axis : x axis, e1 = unit(cross(n, ax)), e2 =
//     cross(n, e1); g_i = rp dot(e_i, w); with a_i = dot(e_i, a), b_i = dot(e_i, b),
//     H11 = (rp rp) ((1 - a1 a1) ila + (1 - b1 b1) ilb) - rp wn, H22 alike with index
//     2, H12 = (rp rp) ((0 - a1 a2) ila + (0 - b1 b2) ilb); det = H11 H22 - H12 H12;
//     d1 = -(g1 H22 - g2 H12) / det, d2 = -(H11 g2 - H12 g1) / det; n+ = unit((n + d1
//     e1) + d2 e2); state(n+).
//     Accepted iff n+, T+, det finite, det > 0, dot(n+, O - M+) > 0, the target faces
//     (point: dot(n+, S - M+) > 0, sky: dot(n+, r) > 0) and T+ < T.  A refused step
//     ends the iteration with the n it had.  M = c + rp n; not finite: Mg.
//     RTW_SPECULAR_NO_GUARD (the native check's second build only) accepts every step.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rtw_temporal.hpp"

namespace rtwsp {

constexpr uint32_t kDefSteps = 2, kMaxSteps = 8;
constexpr uint32_t kPredictOnly = 1u;  // = RTW_MIRROR_PREDICT_ONLY
constexpr uint32_t kMatMetal = 1u;     // = RTW_WMAT_METAL
constexpr double kReflTmin = 0.001;    // a reflected ray's t_min; its t_max is +inf

struct V3 {
  double x, y, z;
};
RTW_TP_HD inline V3 v3(double x, double y, double z) {
  V3 r;
  r.x = x, r.y = y, r.z = z;
  return r;
}
RTW_TP_HD inline V3 ld(const double* p) { return v3(p[0], p[1], p[2]); }
RTW_TP_HD inline bool finite(double x) { return x - x == 0.0; }
RTW_TP_HD inline bool finite3(const V3& a) { return finite(a.x) && finite(a.y) && finite(a.z); }
RTW_TP_HD inline double dot(const V3& a, const V3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RTW_TP_HD inline V3 cross(const V3& a, const V3& b) {
  return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
RTW_TP_HD inline V3 sub(const V3& a, const V3& b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
RTW_TP_HD inline V3 add(const V3& a, const V3& b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
RTW_TP_HD inline V3 madd(const V3& a, double s, const V3& b) { return v3(a.x + s * b.x, a.y + s * b.y, a.z + s * b.z); }
RTW_TP_HD inline V3 msub(const V3& a, double s, const V3& b) { return v3(a.x - s * b.x, a.y - s * b.y, a.z - s * b.z); }
RTW_TP_HD inline V3 divs(const V3& a, double s) { return v3(a.x / s, a.y / s, a.z / s); }
RTW_TP_HD inline double len(const V3& a) { return sqrt(dot(a, a)); }
RTW_TP_HD inline V3 unit(const V3& a) { return divs(a, len(a)); }

// 0 = default; false: out of range.
RTW_TP_HD inline bool resolve(uint32_t steps, uint32_t flags, uint32_t& steps_out) {
  if (steps > kMaxSteps || (flags & ~kPredictOnly) != 0u) return false;
  steps_out = (flags & kPredictOnly) ? 0u : (steps ? steps : kDefSteps);
  return true;
}

// A record counts as a mirror: a hit of the world's list, on the front, whose
// material is metal; kind: rtw_prim_kind (spheres and rects: every kind).
RTW_TP_HD inline bool is_mirror(uint32_t prim, uint32_t n_prims, uint32_t front, uint32_t kind, uint32_t mat_kind) {
  return prim != 0u && prim <= n_prims && front == 1u && mat_kind == kMatMetal && kind <= 4u;
}

// ray: 9 doubles = rtw_ray; p, nrm: the record's.
RTW_TP_HD inline void reflect_ray(const double ray[9], const double p[3], const double nrm[3], double out[9]) {
  const V3 d = ld(ray + 3), n = ld(nrm);
  const double k = 2.0 * dot(d, n);
  out[0] = p[0], out[1] = p[1], out[2] = p[2];
  out[3] = d.x - k * n.x, out[4] = d.y - k * n.y, out[5] = d.z - k * n.z;
  out[6] = ray[6];
  out[7] = kReflTmin;
  out[8] = __builtin_huge_val();
}

RTW_TP_HD inline void prev_normal(const double nrm[3], uint32_t xf_h, const double* v_now, const double* v_prev,
                                  bool moved, double out[3]) {
  double n0 = nrm[0], n1 = nrm[1], n2 = nrm[2];
  if (moved) {
    const int n = (int)rtwr::xform_ops(xf_h);
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
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = (int)rtwk::kMaxXfOps - 1; i >= 0; --i) {
      if (i >= n) continue;
      if (rtwr::xform_op(xf_h, i) != 0u) {
        const double w0 = v_prev[3 * i], w1 = v_prev[3 * i + 1];
        const double a = n0, b = n2;
        n0 = w1 * a + w0 * b;
        n2 = -w0 * a + w1 * b;
      }
    }
  }
  out[0] = n0, out[1] = n1, out[2] = n2;
}

struct State {  // of a normal n on the sphere
  V3 a, b;
  double ila, ilb, wn, T;
};
RTW_TP_HD inline State state_of(const V3& n, const V3& c, double rp, const V3& O, bool tsky, const V3& tg, V3& M) {
  State s;
  M = madd(c, rp, n);
  const V3 va = sub(M, O);
  const double la = len(va);
  s.a = divs(va, la);
  s.ila = 1.0 / la;
  if (tsky) {
    s.b = v3(-tg.x, -tg.y, -tg.z);
    s.ilb = 0.0;
  } else {
    const V3 vb = sub(M, tg);
    const double lb = len(vb);
    s.b = divs(vb, lb);
    s.ilb = 1.0 / lb;
  }
  const V3 w = add(s.a, s.b);
  s.wn = dot(w, n);
  const V3 tang = msub(w, s.wn, n);
  s.T = dot(tang, tang);
  return s;
}

// kind: rtw_prim_kind; rp: the sphere's radius under the previous numbers (not
// read for a rect); tg: S (a point) or, with tsky, the unit direction r;
// steps: Newton steps (0: the predictor alone).  true: out = M; false: out is
// not written and the caller keeps Mg's bytes.
RTW_TP_HD inline bool mirror_point(uint32_t kind, const double Mg_[3], const double ng_[3], double rp, const double O_[3],
                                   bool tsky, const double tg_[3], uint32_t steps, double out[3]) {
  const V3 Mg = ld(Mg_), ng = ld(ng_), O = ld(O_), tg = ld(tg_);
  if (!(finite3(Mg) && finite3(ng) && finite3(O) && finite3(tg))) return false;
  const V3 vo = sub(O, Mg);
  const double cs = dot(divs(vo, len(vo)), ng);
  if (!(finite(cs) && cs > 0.0)) return false;
  if (kind >= 2u) {
    V3 dir;
    if (tsky) {
      const double h = dot(tg, ng);
      if (!(h > 0.0)) return false;
      dir = msub(tg, 2.0 * h, ng);
    } else {
      const double h = dot(sub(tg, Mg), ng);
      if (!(h > 0.0)) return false;
      dir = sub(msub(tg, 2.0 * h, ng), O);
    }
    const double den = dot(dir, ng);
    if (!finite(den) || den == 0.0) return false;
    const double s = dot(sub(Mg, O), ng) / den;
    const V3 M = madd(O, s, dir);
    if (!finite3(M)) return false;
    out[0] = M.x, out[1] = M.y, out[2] = M.z;
    return true;
  }
  if (!(finite(rp) && rp > 0.0)) return false;
  const V3 c = msub(Mg, rp, ng);
  const double kappa = (1.0 / cs + cs) / rp;
  if (!finite(kappa)) return false;
  V3 V;
  if (tsky) {
    const double h = dot(tg, ng);
    V = add(Mg, divs(msub(tg, 2.0 * h, ng), kappa));
  } else {
    const V3 vs = sub(tg, Mg);
    const double q = 1.0 + len(vs) * kappa;
    if (!(finite(q) && q > 0.0)) return false;
    const double h = dot(vs, ng);
    V = add(Mg, divs(msub(vs, 2.0 * h, ng), q));
  }
  V3 n = ng;
  {
    const V3 dv = sub(V, O), oc = sub(O, c);
    const double a = dot(dv, dv), hb = dot(oc, dv), cc = dot(oc, oc) - rp * rp;
    const double disc = hb * hb - a * cc;
    if (disc >= 0.0 && a > 0.0) {
      const double t = (-hb - sqrt(disc)) / a;
      const V3 n0 = unit(madd(oc, t, dv));
      if (t > 0.0 && finite3(n0)) n = n0;
    }
  }
  V3 M;
  State s = state_of(n, c, rp, O, tsky, tg, M);
  for (uint32_t it = 0; it < kMaxSteps; ++it) {
    if (it >= steps) break;
    const V3 ax = (n.x * n.x > 0.5) ? v3(0.0, 1.0, 0.0) : v3(1.0, 0.0, 0.0);
    const V3 e1 = unit(cross(n, ax));
    const V3 e2 = cross(n, e1);
    const V3 w = add(s.a, s.b);
    const double g1 = rp * dot(e1, w), g2 = rp * dot(e2, w);
    const double a1 = dot(e1, s.a), a2 = dot(e2, s.a), b1 = dot(e1, s.b), b2 = dot(e2, s.b);
    const double rr = rp * rp, curv = rp * s.wn;
    const double H11 = rr * ((1.0 - a1 * a1) * s.ila + (1.0 - b1 * b1) * s.ilb) - curv;
    const double H22 = rr * ((1.0 - a2 * a2) * s.ila + (1.0 - b2 * b2) * s.ilb) - curv;
    const double H12 = rr * ((0.0 - a1 * a2) * s.ila + (0.0 - b1 * b2) * s.ilb);
    const double det = H11 * H22 - H12 * H12;
    const double d1 = -(g1 * H22 - g2 * H12) / det, d2 = -(H11 * g2 - H12 * g1) / det;
    const V3 np = unit(madd(madd(n, d1, e1), d2, e2));
    V3 Mp;
    const State sp = state_of(np, c, rp, O, tsky, tg, Mp);
#if !defined(RTW_SPECULAR_NO_GUARD)
    const double fo = dot(np, sub(O, Mp));
    const double ft = tsky ? dot(np, tg) : dot(np, sub(tg, Mp));
    if (!(finite3(np) && finite(sp.T) && finite(det) && det > 0.0 && fo > 0.0 && ft > 0.0 && sp.T < s.T)) break;
#endif
    n = np;
    s = sp;
  }
  M = madd(c, rp, n);
  if (!finite3(M)) return false;
  out[0] = M.x, out[1] = M.y, out[2] = M.z;
  return true;
}

// ---- library internals (rtw_specular_host.cpp), shared by the host and device entries ----
// The checks the two forms share after their own null-pointer rules: alignment, n,
// the options, and no output overlapping an input or the other output (byte ranges;
// NULL buffers left out).  a_bytes / xv_bytes: the previous arrays' sizes.
int check_call(const char* who, const void* rays, const void* hits, const void* hits2_in, uint64_t n,
               const void* cam_prev, const void* a_prev, size_t a_bytes, const void* xv_prev, size_t xv_bytes,
               uint32_t steps, uint32_t flags, const void* prev_p, const void* hits2_out, uint32_t& steps_out);

}  // namespace rtwsp
