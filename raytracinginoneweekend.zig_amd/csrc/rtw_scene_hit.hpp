// rtw_scene_hit.hpp — the closest hit of one ray over a scene's packed sphere
// table, in f64: what scene_query_kernel (rtw_query.hip) and
// scene_guides_kernel (rtw_guides.hip) share, so the two loops cannot drift
// apart.  A wave-uniform loop in table order (scalar record loads) with the tie
// rule on list indices, and the render's NaN rule: a
// lane that met a NaN root runs the reference's literal loop in list order.
// Device code; include after rtw_device.hpp.
#pragma once
#include "rtw_device.hpp"

namespace rtwk {

// What the table loop of scene_closest makes of a NaN root: -inf, which is below every root, so it wins,
// nothing replaces it, and h.t == kNanRoot after the loop says that the lane met one.  fmax returns its other
// argument for a NaN: two instructions among those of a candidate that passed t_min.  (A flag set under
// `root != root` costs a select in the loop header, for EVERY sphere: +1.6 % on scene_guides_kernel.)  A
// t_max of -inf reads as the mark too and takes the sequential loop, which is the reference's: the same answer.
constexpr double kNanRoot = -__builtin_huge_val();

struct SceneHit {
  int pos, orig;  // table position and list index of the winner; -1: a miss
  double t;
};

// Sphere.center / MovingSphere.center (hittable.zig:219-221) of table record k.
__device__ __forceinline__ V3<double> scene_center(const SceneView<double>& S, uint32_t k, uint32_t meta, double time) {
  const double* sp = S.sph + 8 * k;
  V3<double> c = ld3(sp);
  if (meta & kMoving) {
    const double* tg = S.tg + 4 * ((meta >> 2) & 63u);
    c = add(c, mul(ld3(sp + 3), (time - tg[0]) / (tg[1] - tg[0])));
  }
  return c;
}

// Sphere.hit / MovingSphere.hit (hittable.zig:96-116, :166-187) up to the first
// root: false where the discriminant is negative.
__device__ __forceinline__ bool scene_roots(const SceneView<double>& S, uint32_t k, uint32_t meta, const V3<double>& o,
                                            const V3<double>& d, double a, double time, double& hb, double& sq) {
  const V3<double> oc = sub(o, scene_center(S, k, meta, time));
  hb = dot(oc, d);
  const double cc = norm2(oc) - S.sph[8 * k + 6];
  const double disc = hb * hb - a * cc;
  if (disc < 0.0) return false;
  sq = sqrt(disc);
  return true;
}

// HittableList.hit (hittable.zig:231-244) with the initial closest tmax.  The
// reference accepts a NaN root whatever the closest is, and after it every
// later sphere of the LIST whose discriminant is not negative: a lane that met
// one runs that loop literally, in list order (perm).  ANY (occlusion): only
// `pos >= 0` is meaningful; the wave leaves the loop when no lane is without an
// accepted root, and a NaN root is one (the reference accepts it), so an
// occlusion lane never needs the sequential loop.
template <bool ANY>
__device__ __forceinline__ SceneHit scene_closest(const SceneView<double>& S, const V3<double>& o, const V3<double>& d,
                                                  double time, double tmin, double tmax) {
  const double a = norm2(d);
  SceneHit h;
  h.pos = -1, h.orig = -1, h.t = tmax;
  for (uint32_t k = 0; k < S.n; ++k) {  // (wave-uniform) minimal root, ties to the later sphere of the list
    const uint32_t meta = S.meta[k];
    double hb, sq;
    if (!scene_roots(S, k, meta, o, d, a, time, hb, sq)) continue;
    double root = (-hb - sq) / a;
    if (root < tmin) root = (-hb + sq) / a;
    if (root < tmin) continue;
    root = fmax(root, kNanRoot);  // (a NaN root — an overflowing |dir|^2 gives disc = inf - inf — wins and stays)
    const int orig = (int)(meta >> 20);
    if ((root < h.t) | ((root == h.t) & (orig > h.orig))) h.t = root, h.pos = (int)k, h.orig = orig;
    if constexpr (ANY) {
      if (!wany(h.pos < 0)) break;
    }
  }
  if constexpr (!ANY) {
    const bool nan_seen = h.t == kNanRoot;
    if (__builtin_expect(wany(nan_seen), 0)) {
      if (nan_seen) {  // Sphere.hit's own acceptance, against the closest so far
        h.pos = -1, h.orig = -1, h.t = tmax;
        for (uint32_t i = 0; i < S.n; ++i) {
          const uint32_t k = S.perm[i];
          double hb, sq;
          if (!scene_roots(S, k, S.meta[k], o, d, a, time, hb, sq)) continue;
          double root = (-hb - sq) / a;
          if (root < tmin || h.t < root) {
            root = (-hb + sq) / a;
            if (root < tmin || h.t < root) continue;
          }
          h.t = root, h.pos = (int)k, h.orig = (int)i;
        }
      }
    }
  }
  return h;
}

}  // namespace rtwk
