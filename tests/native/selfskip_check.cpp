// selfskip_check.cpp — rtws::leaves (csrc/rtw_selfskip.hpp) against the reference's literal f64 sphere test.
//
// Every case is a ray that starts on (or within rounding of, or a controlled distance inside) a sphere, made
// the way the kernel makes it: a previous ray is intersected with the sphere by the literal test, the hit
// point is o + d * t with that rounded root, and the new direction is Material.scatter's.  The verdict is the
// oracle's test (oracle/tierb_core.h `test`, f64 branch: hittable.zig:96-116) restated here and nothing else:
//   violation = the rule fires and the literal test accepts the sphere.
// usage: selfskip_check [cases] [seed]; prints "selfskip_check: cases N fired F violations V cover_leaving L
// cover_fired C"; exit status 1 when V > 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "rtw_selfskip.hpp"

namespace {

struct V {
  double x, y, z;
};
V add(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V sub(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V mul(V a, double t) { return {a.x * t, a.y * t, a.z * t}; }
V divs(V a, double t) { return {a.x / t, a.y / t, a.z / t}; }
double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }  // left to right (vec.zig:20-22)
double norm2(V a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
V normalized(V v) {
  const double n = std::sqrt(norm2(v));
  return n == 0.0 ? v : divs(v, n);
}

struct Rng {
  uint64_t s;
  uint64_t next() {
    s += 0x9e3779b97f4a7c15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
  }
  double u() { return (double)(next() >> 11) * 0x1p-53; }            // [0, 1)
  double r(double a, double b) { return a + u() * (b - a); }
  double lg(double a, double b) { return std::exp(r(std::log(a), std::log(b))); }  // log-uniform
  uint32_t k(uint32_t n) { return (uint32_t)(next() % n); }
  V ball() {
    for (;;) {
      const V p = {r(-1, 1), r(-1, 1), r(-1, 1)};
      if (norm2(p) < 1.0 && norm2(p) > 1e-12) return p;
    }
  }
  V unit() { return normalized(ball()); }
};

// The first values of Sphere.hit / MovingSphere.hit for the NEXT segment, as the test computes them.
struct Quad {
  double hb, cc, a;
};
Quad quad(V o, V d, V centre, double r2) {
  const V oc = sub(o, centre);
  return {dot(oc, d), norm2(oc) - r2, norm2(d)};
}
// The literal test's verdict on them (tierb_core.h `test`, f64): true = the sphere is rejected.
bool literal_rejects(double half_b, double c, double a, double tmin, double tmax) {
  const double disc = half_b * half_b - a * c;
  if (disc < 0) return true;
  const double sq = std::sqrt(disc);
  double root = (-half_b - sq) / a;
  if (root < tmin || tmax < root) {
    root = (-half_b + sq) / a;
    if (root < tmin || tmax < root) return true;
  }
  return false;
}
// The accepted root of the literal test (the previous segment's hit); false: no hit.
bool literal_root(V o, V d, V centre, double r2, double tmin, double& root) {
  const Quad q = quad(o, d, centre, r2);
  const double disc = q.hb * q.hb - q.a * q.cc;
  if (disc < 0) return false;
  const double sq = std::sqrt(disc);
  root = (-q.hb - sq) / q.a;
  if (root < tmin) {
    root = (-q.hb + sq) / q.a;
    if (root < tmin) return false;
  }
  return true;
}

V reflect(V v, V n) { return sub(v, mul(n, 2 * dot(v, n))); }
V refract(V uv, V n, double eta) {
  const double cos_theta = std::fmin(dot(mul(uv, -1), n), 1.0);
  const V perp = mul(add(uv, mul(n, cos_theta)), eta);
  const V par = mul(n, -std::sqrt(std::fabs(1 - norm2(perp))));
  return add(perp, par);
}

struct Tally {
  unsigned long long cases = 0, fired = 0, viol = 0, cover_leaving = 0, cover_fired = 0;
  int shown = 0;
};

void judge(Tally& t, V o, V d, V centre, double r2, double tmin, bool cover) {
  const Quad q = quad(o, d, centre, r2);
  const bool fire = rtws::leaves(q.hb, q.cc, q.a, tmin);
  const bool rej = literal_rejects(q.hb, q.cc, q.a, tmin, INFINITY);
  t.cases++;
  t.fired += fire;
  if (cover && q.hb > 0) {
    t.cover_leaving++;
    t.cover_fired += fire;
  }
  if (fire && !rej) {
    t.viol++;
    if (t.shown++ < 5)
      std::printf("violation: hb %.17g cc %.17g a %.17g tmin %.17g\n", q.hb, q.cc, q.a, tmin);
  }
}

// A sphere, a ray that hits it (grazing by `graze` in (0, 1]: 1 = through the centre), the hit point built as
// the kernel builds it, and the scattered direction of material `kind`.
void scatter_case(Tally& t, Rng& g, bool cover) {
  const double cscale = cover ? 11.0 : g.lg(1e-2, 0x1p20);
  V c0 = {g.r(-cscale, cscale), cover ? g.r(0.2, 1.0) : g.r(-cscale, cscale), g.r(-cscale, cscale)};
  double rad = cover ? (g.k(8) == 0 ? 1.0 : 0.2) : g.lg(1e-3, 99.0);
  const bool hollow = !cover ? g.k(4) == 0 : g.k(40) == 0;
  if (hollow) rad = -rad;
  const double r2 = rad * rad;
  V centre = c0;
  if (g.k(4) == 0) {  // a moving sphere at a shutter end or inside: centre(time) = c0 + dc * frac
    const double t0 = g.r(0, 0.5), t1 = t0 + g.r(0.1, 1.0);
    const double time = g.k(3) == 0 ? t0 : (g.k(2) ? t1 : g.r(t0, t1));
    const double frac = (time - t0) / (t1 - t0);
    const V dc = {0.0, g.r(0, 0.5), g.k(2) ? 0.0 : g.r(-0.5, 0.5)};
    centre = add(c0, mul(dc, frac));
  }
  const double tmin = cover ? 1e-3 : g.lg(1e-6, 1e-1);
  const double R = std::fabs(rad);
  // the previous ray: from outside (a point at distance > R) or from inside (refraction), aimed at a point
  // at distance graze_r <= R from the centre, perpendicular offsets down to grazing incidence
  const bool inside = g.k(4) == 0;
  const V dir0 = g.unit();
  V perp = normalized(sub(g.unit(), mul(dir0, 0.0)));
  perp = normalized(sub(perp, mul(dir0, dot(perp, dir0))));
  const double off = g.k(3) == 0 ? R * (1.0 - g.lg(1e-16, 1e-2)) : R * g.u();  // grazing / anywhere
  const double back = inside ? g.r(0.0, 0.5) * std::sqrt(std::fmax(R * R - off * off, 0.0)) : R * g.lg(1.001, 1e3);
  const V o0 = add(centre, add(mul(perp, off), mul(dir0, -back)));
  const V d0 = mul(dir0, cover ? g.lg(0.5, 2.0) : g.lg(1e-6, 1e6));
  double root;
  if (!literal_root(o0, d0, centre, r2, tmin, root)) return;
  const V p = add(o0, mul(d0, root));  // ray.at(t)
  const V outward = divs(sub(p, centre), rad);
  const bool front = dot(outward, d0) < 0;
  const V normal = front ? outward : mul(outward, -1);
  const uint32_t kind = g.k(cover ? 10 : 6);
  V nd;
  if (kind == 0 || kind >= 6) {  // Lambertian; adversarial: normal + unit nearly cancelling
    V uv = g.unit();
    if (!cover && g.k(2)) uv = normalized(add(mul(normal, -1), mul(g.ball(), g.lg(1e-9, 1e-2))));
    nd = add(normal, uv);
    if (std::fabs(nd.x) < 1e-8 && std::fabs(nd.y) < 1e-8 && std::fabs(nd.z) < 1e-8) nd = normal;
  } else if (kind <= 2) {  // Metal, fuzz 0, 1 or between
    const double fuzz = kind == 1 ? (g.k(2) ? 0.0 : 1.0) : g.u();
    nd = add(reflect(normalized(d0), normal), mul(g.ball(), fuzz));
  } else {  // Dielectric: reflection or refraction, from outside and from inside
    const double ir = 1.5, ratio = front ? 1 / ir : ir;
    const V ud = normalized(d0);
    const double cos_theta = std::fmin(dot(mul(ud, -1), normal), 1.0);
    const double sin_theta = std::sqrt(1 - cos_theta * cos_theta);
    const bool refr = ratio * sin_theta <= 1 && g.k(2);
    nd = refr ? refract(ud, normal, ratio) : reflect(ud, normal);
  }
  judge(t, p, nd, centre, r2, tmin, cover);
}

// Around the rule's own edges: origins a controlled distance inside or outside the surface
// (cc = -theta * tmin * hb for theta up to 30: where a looser constant is wrong), |d|^2 across and beyond
// [2^-40, 2^40], hb up to and past 2^50 tmin a, tmin beyond its range, and NaN / infinite operands.
void edge_case(Tally& t, Rng& g) {
  const double R = g.lg(1e-3, 99.0), r2 = R * R;
  const double cs = g.lg(1e-2, 0x1p20);
  const V centre = {g.r(-cs, cs), g.r(-cs, cs), g.r(-cs, cs)};
  const double tmin = g.k(8) == 0 ? g.lg(1e-40, 1e40) : g.lg(1e-6, 1e-1);
  const V n = g.unit();
  const double dlen = g.k(6) == 0 ? g.lg(1e-25, 1e25) : g.lg(1e-4, 1e4);
  // direction with a chosen cosine to the outward normal (grazing to normal)
  V tang = g.unit();
  tang = normalized(sub(tang, mul(n, dot(tang, n))));
  const double cosv = g.k(2) ? g.lg(1e-12, 1.0) : g.u();
  const V d = mul(add(mul(n, cosv), mul(tang, std::sqrt(std::fmax(1 - cosv * cosv, 0.0)))), dlen);
  // radial position: |oc| = R + e with cc ~ 2 R e = -theta * tmin * hb, hb ~ R cosv dlen
  const double theta = g.k(3) == 0 ? g.r(0.0, 2.0) : g.r(0.0, 30.0);
  const double e = -theta * tmin * (cosv * dlen) / 2.0;
  V o = add(centre, mul(n, R + e));
  if (g.k(64) == 0) o.x = g.k(2) ? NAN : INFINITY;
  V dd = d;
  if (g.k(64) == 0) dd.y = g.k(2) ? NAN : -INFINITY;
  judge(t, o, dd, centre, r2, g.k(128) == 0 ? NAN : tmin, false);
  // far along the ray behind the sphere's far side: hb huge against tmin * a
  if (g.k(4) == 0) {
    const double far = g.lg(1.0, 1e15);
    judge(t, add(o, mul(normalized(d), far)), mul(d, g.lg(1e-8, 1.0)), centre, r2, tmin, false);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const unsigned long long n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 12000000ull;
  Rng g{argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1ull};
  Tally t;
  while (t.cases < n) {
    scatter_case(t, g, true);   // the cover-like generator
    scatter_case(t, g, false);  // the adversarial one
    edge_case(t, g);
  }
  // fixed cases the rule must refuse: a ray that enters, NaNs, a and tmin out of range
  unsigned long long refused_bad = 0;
  refused_bad += rtws::leaves(-1.0, 0.0, 1.0, 1e-3);
  refused_bad += rtws::leaves(0.0, 0.0, 1.0, 1e-3);
  refused_bad += rtws::leaves(NAN, 0.0, 1.0, 1e-3);
  refused_bad += rtws::leaves(1.0, NAN, 1.0, 1e-3);
  refused_bad += rtws::leaves(1.0, 0.0, NAN, 1e-3);
  refused_bad += rtws::leaves(1.0, 0.0, 1.0, NAN);
  refused_bad += rtws::leaves(1.0, 0.0, 0x1p41, 1e-3);
  refused_bad += rtws::leaves(1e-20, 0.0, 0x1p-41, 1e-3);
  refused_bad += rtws::leaves(1.0, 0.0, 1.0, 0.0);
  refused_bad += rtws::leaves(1.0, 0.0, 1.0, -1e-3);
  refused_bad += rtws::leaves(INFINITY, 0.0, 1.0, 1e-3);
  refused_bad += !rtws::leaves(1.0, 0.0, 1.0, 1e-3);  // and the plain leaving ray fires
  t.viol += refused_bad;
  std::printf("selfskip_check: cases %llu fired %llu violations %llu cover_leaving %llu cover_fired %llu\n", t.cases,
              t.fired, t.viol, t.cover_leaving, t.cover_fired);
  return t.viol ? 1 : 0;
}
