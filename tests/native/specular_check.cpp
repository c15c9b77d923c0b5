// specular_check.cpp — csrc/rtw_specular.hpp on the CPU, no HIP:
//  1. nothing moved: with the same camera and the same numbers the mirror point
//     is the record's own point (spheres, moving spheres, rects under Translate +
//     RotateY, sky targets), to 1e-9;
//  2. rects: the law of reflection holds at the result to 1e-9 on fuzzed planes;
//  3. spheres: a census against an independent solve (damped descent on the path
//     length, its step damped on the gradient, written here a second time) on the cover camera at 1200 x 675, a
//     mirror sphere orbiting the y axis over a ground plane: r = 1 and r = 0.2 at
//     1 degree per frame (asserted) and r = 1 at 5 degrees (printed; there the
//     acceptance guard's promises are asserted, which a header built with
//     RTW_SPECULAR_NO_GUARD must break);
//  4. every fallback refuses (the caller keeps the surface point's bytes);
//  5. steps 1 and 8 stay finite.
// Prints "specular_check: bad B/N"; exit status 1 when B > 0.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "rtw_specular.hpp"

namespace {

long g_bad = 0, g_checks = 0;
void check(bool ok, const char* what) {
  ++g_checks;
  if (!ok) {
    if (g_bad < 20) std::printf("FAIL: %s\n", what);
    ++g_bad;
  }
}

// ---- the check's own vectors (not the header's) ----
struct P3 {
  double x, y, z;
};
P3 operator+(P3 a, P3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
P3 operator-(P3 a, P3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
P3 operator*(double s, P3 a) { return {s * a.x, s * a.y, s * a.z}; }
double dt(P3 a, P3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
P3 cr(P3 a, P3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double nm(P3 a) { return std::sqrt(dt(a, a)); }
P3 un(P3 a) { return (1.0 / nm(a)) * a; }
P3 roty(P3 p, double ang) {  // RotateY's forward map
  const double s = std::sin(ang), c = std::cos(ang);
  return {c * p.x + s * p.z, p.y, -s * p.x + c * p.z};
}

struct Cam {
  double origin[3], h[3], v[3], llc[3];
};
Cam cover_camera() {  // lookfrom (13, 2, 3), lookat 0, vfov 20, 16:9, focus 10
  const P3 from{13, 2, 3}, at{0, 0, 0}, up{0, 1, 0};
  const double vh = 2.0 * std::tan(20.0 * M_PI / 360.0), vw = vh * 16.0 / 9.0, fd = 10.0;
  const P3 w = un(from - at), u = un(cr(up, w)), v = cr(w, u);
  const P3 H = (fd * vw) * u, V = (fd * vh) * v, L = from - 0.5 * H - 0.5 * V - fd * w;
  Cam c;
  c.origin[0] = from.x, c.origin[1] = from.y, c.origin[2] = from.z;
  c.h[0] = H.x, c.h[1] = H.y, c.h[2] = H.z;
  c.v[0] = V.x, c.v[1] = V.y, c.v[2] = V.z;
  c.llc[0] = L.x, c.llc[1] = L.y, c.llc[2] = L.z;
  return c;
}
constexpr int kW = 1200, kH = 675;

bool pixel_of(const rtwt::Proj& pr, P3 p, double& fx, double& fy) {
  // the projection stated here: d0 + s h + t v = mu (p - origin)
  const P3 q{p.x - pr.origin[0], p.y - pr.origin[1], p.z - pr.origin[2]};
  const P3 h{pr.h[0], pr.h[1], pr.h[2]}, v{pr.v[0], pr.v[1], pr.v[2]}, d0{pr.d0[0], pr.d0[1], pr.d0[2]};
  const P3 n = cr(h, v);
  const double det = dt(q, n);
  if (!(std::fabs(det) > 0)) return false;
  const double mu = dt(d0, n) / det, s = -dt(q, cr(d0, v)) / det, t = -dt(q, cr(h, d0)) / det;
  if (!(mu > 0)) return false;
  fx = s * (kW - 1) - 0.5;
  fy = ((kH - 1) + 0.5) - t * (kH - 1);
  return true;
}

// ---- the independent solve: damped descent on f(n) = |M - O| + |M - S| (sky: |M - O| - dot(M, r)) ----
struct Target {
  bool sky;
  P3 t;
};
double path_len(P3 c, double r, P3 n, P3 O, const Target& T) {
  const P3 M = c + r * n;
  return nm(M - O) + (T.sky ? -dt(M, T.t) : nm(M - T.t));
}
P3 tang_grad(P3 c, double r, P3 n, P3 O, const Target& T) {
  const P3 M = c + r * n;
  const P3 g = un(M - O) + (T.sky ? (-1.0) * T.t : un(M - T.t));
  return g - dt(g, n) * n;
}
// The step is damped on the gradient itself (halved until the tangential gradient shrinks), since a decrease of
// f below its rounding cannot be seen in f.
bool brute(P3 c, double r, P3 n0, P3 O, const Target& T, P3& n_out) {
  P3 n = n0;
  double step = 1.0;
  P3 g = tang_grad(c, r, n, O, T);
  double gn = nm(g);
  for (int it = 0; it < 20000; ++it) {
    if (gn < 1e-12) {
      n_out = n;
      return true;
    }
    bool moved = false;
    for (int k = 0; k < 60; ++k) {
      const P3 n1 = un(n - step * g);
      const P3 g1 = tang_grad(c, r, n1, O, T);
      const double gn1 = nm(g1);
      if (gn1 < gn) {
        n = n1, g = g1, gn = gn1, moved = true;
        step *= 1.25;
        break;
      }
      step *= 0.5;
    }
    if (!moved) return false;
  }
  return false;
}

bool call(uint32_t kind, P3 Mg, P3 ng, double rp, P3 O, const Target& T, uint32_t steps, P3& out) {
  const double a[3] = {Mg.x, Mg.y, Mg.z}, b[3] = {ng.x, ng.y, ng.z}, o[3] = {O.x, O.y, O.z}, t[3] = {T.t.x, T.t.y, T.t.z};
  double m[3] = {Mg.x, Mg.y, Mg.z};
  const bool ok = rtwsp::mirror_point(kind, a, b, rp, o, T.sky, t, steps, m);
  out = {m[0], m[1], m[2]};
  return ok;
}

struct Dist {
  std::vector<double> e;
  void add(double x) { e.push_back(x); }
  double mean() const {
    double s = 0;
    for (double x : e) s += x;
    return e.empty() ? 0 : s / e.size();
  }
  double q(double f) {
    if (e.empty()) return 0;
    std::sort(e.begin(), e.end());
    return e[std::min(e.size() - 1, (size_t)(f * e.size()))];
  }
  double within(double tol) const {
    size_t k = 0;
    for (double x : e) k += x <= tol;
    return e.empty() ? 0 : (double)k / e.size();
  }
};

// One set-up of the census.  assert_accuracy: the 1-degree assertions; else the guard's promises.
void census(const char* name, double radius, double deg, bool assert_accuracy, uint32_t seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const Cam cam = cover_camera();
  const rtwt::Proj pr = rtwt::make_proj(cam.origin, cam.h, cam.v, cam.llc);
  const P3 O{cam.origin[0], cam.origin[1], cam.origin[2]};
  const double th = deg * M_PI / 180.0;
  const int N = 2000;
  int left_out = 0, refused = 0, broke = 0;
  Dist e_newton, e_pred, e_surf;
  for (int k = 0; k < N; ++k) {
    // the sphere now: on the ground, somewhere in the camera's view
    const double rho = 1.0 + 5.0 * U(rng), phi = (U(rng) - 0.5) * 1.6;
    const P3 c_now{rho * std::cos(phi), radius, rho * std::sin(phi)};
    // a point of it as a frame samples it: uniform over the sphere's image (a pixel is a case), not over its
    // surface, which would count the rim, a few pixels wide, as heavily as the face
    P3 n;
    {
      const P3 w = un(c_now - O), u = un(cr(P3{0, 1, 0}, w)), v = cr(w, u);
      double a, b;
      do a = 2 * U(rng) - 1, b = 2 * U(rng) - 1;
      while (a * a + b * b >= 0.999);
      const P3 dir = un(c_now + (radius * a) * u + (radius * b) * v - O), oc = O - c_now;
      const double hb = dt(oc, dir), disc = hb * hb - (dt(oc, oc) - radius * radius);
      if (!(disc > 0)) {  // (the disc's edge seen past the silhouette)
        ++left_out;
        continue;
      }
      n = un(oc + (-hb - std::sqrt(disc)) * dir);
    }
    const P3 M = c_now + radius * n, d = M - O, refl = d - (2 * dt(d, n)) * n;
    Target T;
    if (refl.y < -1e-3 * nm(refl)) {  // the ground plane y = 0, which the orbit leaves where it is
      T.sky = false, T.t = M + (-M.y / refl.y) * refl;
    } else {
      T.sky = true, T.t = un(refl);
    }
    const P3 c_prev = roty(c_now, -th);  // last frame's centre; no transform chain: the normal stays
    const P3 Mg = c_prev + radius * n;
    P3 nb;
    const bool solved = brute(c_prev, radius, n, O, T, nb);
    const P3 Mb = c_prev + radius * nb;
    double bx, by;
    const bool visible = solved && dt(nb, O - Mb) > 0 && (T.sky ? dt(nb, T.t) > 0 : dt(nb, T.t - Mb) > 0) && pixel_of(pr, Mb, bx, by);
    if (!visible) {
      ++left_out;
      continue;
    }
    P3 m2, m0;
    const bool ok2 = call(0, Mg, n, radius, O, T, 2, m2), ok0 = call(0, Mg, n, radius, O, T, 0, m0);
    if (!ok2 || !ok0) ++refused;  // (the surface point stands in, as in the library)
    double x, y;
    auto err = [&](P3 p) { return pixel_of(pr, p, x, y) ? std::hypot(x - bx, y - by) : 1e9; };
    e_newton.add(err(m2)), e_pred.add(err(m0)), e_surf.add(err(Mg));
    if (!assert_accuracy && ok2 && ok0) {
      // what the guard promises of an accepted iteration: no larger residual than the predictor's, and a point that
      // faces the camera and the target whenever the predictor's did
      const P3 n2 = un(m2 - c_prev), np0 = un(m0 - c_prev);
      const double t2 = nm(tang_grad(c_prev, radius, n2, O, T)), t0 = nm(tang_grad(c_prev, radius, np0, O, T));
      auto faces = [&](P3 nn, P3 p) { return dt(nn, O - p) > 0 && (T.sky ? dt(nn, T.t) > 0 : dt(nn, T.t - p) > 0); };
      const bool fine = std::isfinite(t2) && t2 <= t0 * (1 + 1e-9) + 1e-15 && (!faces(np0, m0) || faces(n2, m2));
      if (!fine) ++broke;
    }
  }
  const int used = N - left_out;
  std::printf("census %-14s r=%.1f %g deg: used %d left out %d refused %d\n", name, radius, deg, used, left_out, refused);
  std::printf("  px error   mean      p50       p95       p99       max       within 0.1 px\n");
  auto row = [](const char* nm_, Dist& d) {
    std::printf("  %-9s %9.3g %9.3g %9.3g %9.3g %9.3g   %.4f\n", nm_, d.mean(), d.q(0.5), d.q(0.95), d.q(0.99), d.q(1.0), d.within(0.1));
  };
  row("surface", e_surf), row("predictor", e_pred), row("newton 2", e_newton);
  check(left_out * 50 <= N, "census: more than 2 % of the cases left out");
  if (assert_accuracy) {
    check(e_newton.within(0.1) >= 0.95, "census: fewer than 95 % within 0.1 px of the solve");
    check(e_pred.mean() < e_surf.mean(), "census: the predictor's mean error is not below the surface point's");
  } else {
    std::printf("  guard promises broken: %d\n", broke);
    check(broke == 0, "census: an accepted iteration broke the guard's promises");
  }
}

void nothing_moved() {
  std::mt19937_64 rng(21);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  for (int k = 0; k < 4000; ++k) {
    const int kind = k % 4;  // 0 sphere, 1 moving sphere, 2 rect under Translate + RotateY, 3 sphere with a sky target
    const P3 O{8 + 6 * U(rng), 1 + 3 * U(rng), -3 + 6 * U(rng)};
    double p[3], nrm[3], u = 0, v = 0, r_prev[11] = {0}, time = U(rng);
    uint32_t pk = 0, xf_h = 0;
    double xv[12] = {0};
    if (kind == 2) {
      // XZ rect y = k under op 0 Translate (outermost), op 1 RotateY
      const double a[9] = {-2, 2, -1.5, 1.5, 0.3 + U(rng), 0, 0, 0, 0};
      rtwr::fill_record(3u, a, r_prev);
      pk = 3u;
      const double ang = 2 * U(rng) - 1;
      xf_h = 2u | (0u << 8) | (1u << 12);
      xv[0] = U(rng), xv[1] = U(rng), xv[2] = U(rng);
      xv[3] = std::sin(ang), xv[4] = std::cos(ang), xv[5] = ang;
      u = U(rng), v = U(rng);
      const P3 po{a[0] + u * (a[1] - a[0]), a[4], a[2] + v * (a[3] - a[2])};
      const P3 pw = roty(po, ang) + P3{xv[0], xv[1], xv[2]};
      const P3 nw = roty(P3{0, 1, 0}, ang);
      p[0] = pw.x, p[1] = pw.y, p[2] = pw.z, nrm[0] = nw.x, nrm[1] = nw.y, nrm[2] = nw.z;
    } else {
      const P3 c0{4 * U(rng), 1, 2 * U(rng) - 1}, c1 = c0 + P3{0.3 * U(rng), 0.5 * U(rng), 0};
      const double rad = 0.2 + U(rng);
      const double a[9] = {c0.x, c0.y, c0.z, kind == 1 ? c1.x : c0.x, kind == 1 ? c1.y : c0.y, kind == 1 ? c1.z : c0.z, rad, 0, 1};
      pk = kind == 1 ? 1u : 0u;
      rtwr::fill_record(pk, a, r_prev);
      const P3 c = kind == 1 ? c0 + time * (c1 - c0) : c0;
      P3 n;
      for (;;) {
        n = un(P3{2 * U(rng) - 1, 2 * U(rng) - 1, 2 * U(rng) - 1});
        if (dt(n, un(O - (c + rad * n))) > 0.1) break;
      }
      const P3 pw = c + rad * n;
      p[0] = pw.x, p[1] = pw.y, p[2] = pw.z, nrm[0] = n.x, nrm[1] = n.y, nrm[2] = n.z;
    }
    const P3 P{p[0], p[1], p[2]}, Nn{nrm[0], nrm[1], nrm[2]};
    if (!(dt(Nn, un(O - P)) > 0.05)) continue;  // (a rect seen from behind is no mirror record)
    const P3 d = P - O, refl = d - (2 * dt(d, Nn)) * Nn;
    Target T;
    T.sky = kind == 3;
    T.t = T.sky ? un(refl) : P + (0.5 + 3 * U(rng)) * refl;
    double Mg[3], ng[3];
    rtwt::prev_point(p, nrm, u, v, 1u, pk, r_prev, xf_h, xv, xv, time, true, Mg);
    rtwsp::prev_normal(nrm, xf_h, xv, xv, true, ng);
    P3 out;
    const bool ok = call(pk, P3{Mg[0], Mg[1], Mg[2]}, P3{ng[0], ng[1], ng[2]}, r_prev[6], O, T, 2, out);
    check(ok && nm(out - P) <= 1e-9, "nothing moved: the mirror point is not the record's point");
  }
}

void rect_accuracy() {
  std::mt19937_64 rng(22);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  for (int k = 0; k < 4000; ++k) {
    const P3 ng = un(P3{U(rng), U(rng), U(rng)}), Mg{3 * U(rng), 3 * U(rng), 3 * U(rng)};
    P3 O = Mg + 5.0 * P3{U(rng), U(rng), U(rng)}, S = Mg + 5.0 * P3{U(rng), U(rng), U(rng)};
    if (dt(O - Mg, ng) < 0.2) O = O + (0.2 - dt(O - Mg, ng) + std::fabs(U(rng))) * ng;
    if (dt(S - Mg, ng) < 0.2) S = S + (0.2 - dt(S - Mg, ng) + std::fabs(U(rng))) * ng;
    Target T;
    T.sky = (k & 3) == 3;
    T.t = T.sky ? un(S - Mg) : S;
    P3 M;
    const bool ok = call(2u + (uint32_t)(k % 3), Mg, ng, 0.0, O, T, 2, M);
    const P3 a = un(O - M), b = T.sky ? T.t : un(S - M), w = a + b;
    const P3 tang = w - dt(w, ng) * ng;
    check(ok && std::fabs(dt(M - Mg, ng)) <= 1e-9 && nm(tang) <= 1e-9, "rect: the law of reflection does not hold");
  }
}

void fallbacks() {
  const double inf = HUGE_VAL, nan = std::nan("");
  const P3 Mg{1, 2, 0.5}, ng{0, 1, 0}, O{3, 5, 1}, S{-1, 4, 2};
  P3 out;
  Target T{false, S};
  for (uint32_t kind : {0u, 1u, 2u, 3u, 4u}) {
    check(call(kind, Mg, ng, 1.0, O, T, 2, out), "fallbacks: the base case must not refuse");
    check(!call(kind, Mg, ng, 1.0, P3{3, 1, 1}, T, 2, out), "a camera behind the tangent plane");
    check(!call(kind, Mg, ng, 1.0, P3{3, 2, 1}, T, 2, out), "a camera on the tangent plane");
    for (double bad : {inf, -inf, nan}) {
      check(!call(kind, P3{bad, 2, 0.5}, ng, 1.0, O, T, 2, out), "a non-finite Mg");
      check(!call(kind, Mg, P3{0, bad, 0}, 1.0, O, T, 2, out), "a non-finite normal");
      check(!call(kind, Mg, ng, 1.0, P3{3, 5, bad}, T, 2, out), "a non-finite camera");
      check(!call(kind, Mg, ng, 1.0, O, Target{false, P3{bad, 4, 2}}, 2, out), "a non-finite target");
      check(!call(kind, Mg, ng, 1.0, O, Target{true, P3{0, bad, 0}}, 2, out), "a non-finite sky direction");
      if (kind <= 1u) check(!call(kind, Mg, ng, bad, O, T, 2, out), "a non-finite radius");
    }
    if (kind <= 1u) {
      check(!call(kind, Mg, ng, 0.0, O, T, 2, out), "radius 0");
      check(!call(kind, Mg, ng, -1.0, O, T, 2, out), "a negative radius");
    } else {
      check(!call(kind, Mg, ng, 0.0, O, Target{false, P3{-1, 2, 2}}, 2, out), "a target on the plane");
      check(!call(kind, Mg, ng, 0.0, O, Target{false, P3{-1, 1, 2}}, 2, out), "a target behind the plane");
      check(!call(kind, Mg, ng, 0.0, O, Target{true, P3{1, 0, 0}}, 2, out), "a sky direction in the plane");
    }
  }
  // the host entry's use: the caller's point stays when the call refuses
  double m[3] = {7, 8, 9};
  const double a[3] = {1, 2, 0.5}, b[3] = {0, 1, 0}, o[3] = {3, 1, 1}, t[3] = {-1, 4, 2};
  check(!rtwsp::mirror_point(0u, a, b, 1.0, o, false, t, 2, m) && m[0] == 7 && m[1] == 8 && m[2] == 9, "a refusal writes nothing");
}

void step_counts() {
  std::mt19937_64 rng(23);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  for (int k = 0; k < 4000; ++k) {
    const P3 ng = un(P3{U(rng), U(rng), U(rng)}), Mg{3 * U(rng), 3 * U(rng), 3 * U(rng)};
    const P3 O = Mg + 8.0 * P3{U(rng), U(rng), U(rng)}, S = Mg + 8.0 * P3{U(rng), U(rng), U(rng)};
    const double rad = 0.05 + 2 * std::fabs(U(rng));
    Target T;
    T.sky = (k & 3) == 3;
    T.t = T.sky ? un(S - Mg) : S;
    for (uint32_t steps : {1u, 8u}) {
      P3 M{0, 0, 0};
      const bool ok = call((uint32_t)(k & 1), Mg, ng, rad, O, T, steps, M);
      check(!ok || (std::isfinite(M.x) && std::isfinite(M.y) && std::isfinite(M.z)), "steps 1 / 8: a result that is not finite");
      const P3 c = Mg - rad * ng;
      check(!ok || std::fabs(nm(M - c) - rad) <= 1e-9 * (1 + rad), "steps 1 / 8: a result off the sphere");
    }
  }
  uint32_t s = 99;
  check(rtwsp::resolve(0, 0, s) && s == 2 && rtwsp::resolve(8, 0, s) && s == 8 && rtwsp::resolve(5, 1, s) && s == 0, "resolve");
  check(!rtwsp::resolve(9, 0, s) && !rtwsp::resolve(0, 2, s), "resolve refuses");
}

}  // namespace

int main() {
  nothing_moved();
  rect_accuracy();
  census("1 degree", 1.0, 1.0, true, 31);
  census("1 degree", 0.2, 1.0, true, 32);
  census("5 degrees", 1.0, 5.0, false, 33);
  fallbacks();
  step_counts();
  std::printf("specular_check: bad %ld/%ld\n", g_bad, g_checks);
  return g_bad ? 1 : 0;
}
