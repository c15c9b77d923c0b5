// tri_check — csrc/rtw_tri.hpp (the triangle primitive's arithmetic, DESIGN.md
// §22) on the host, with a plain C++ compiler and -ffp-contract=off:
//   1. axis-aligned triangles, all three axes and both windings: n is exactly
//      +-e_k with +0 zeros, t is bitwise the rect's (k - o_k) / d_k, and the hit
//      point and the ray-facing normal are bitwise the rect's;
//   2. watertightness: closed meshes (a tetrahedron, an icosahedron, a jittered
//      level-2 icosphere) and planar quads split along a diagonal, with rays
//      aimed exactly at, and a few ulps beside, points on edges and vertices:
//      every ray hits at least one triangle;
//   3. barycentrics: |v0 + u (v1 - v0) + v (v2 - v0) - p| against the bound
//      derived in DESIGN.md §22 (reported as the largest error / bound);
//   4. boxes: rtw_world_box.hpp prim_box == rtwr::prim_box for kind 5, bit for
//      bit, through chains of 1-4 ops, and the box holds the moved vertices;
//   5. degenerate and non-finite triangles are reported by derive.
// Prints "tri_check: checks N violations M bary_ratio R"; exit status 1 on a violation.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "rtw_hip.h"
#include "rtw_tri.hpp"
#include "rtw_world_box.hpp"
#include "rtw_world_refit.hpp"

static unsigned long long g_checks = 0, g_viol = 0;
#define CHECK(c, ...)                       \
  do {                                      \
    ++g_checks;                             \
    if (!(c)) {                             \
      if (++g_viol <= 10) {                 \
        fprintf(stderr, "VIOLATION: ");     \
        fprintf(stderr, __VA_ARGS__);       \
        fprintf(stderr, "\n");              \
      }                                     \
    }                                       \
  } while (0)

static uint64_t bits(double x) {
  uint64_t u;
  std::memcpy(&u, &x, 8);
  return u;
}
static double step(double x, int ulps) {
  for (int i = 0; i < std::abs(ulps); ++i) x = std::nextafter(x, ulps > 0 ? INFINITY : -INFINITY);
  return x;
}

struct P3 {
  double x, y, z;
};
struct Mesh {
  std::vector<P3> v;
  std::vector<int> f;  // three per face
};

static bool hits_any(const Mesh& m, const P3& o, const P3& d) {
  for (size_t i = 0; i + 2 < m.f.size(); i += 3) {
    double a[9];
    for (int k = 0; k < 3; ++k) a[3 * k] = m.v[m.f[i + k]].x, a[3 * k + 1] = m.v[m.f[i + k]].y, a[3 * k + 2] = m.v[m.f[i + k]].z;
    double n[3], h, t;
    if (!rtwtri::derive(a, n, h)) continue;
    if (rtwtri::root(a, n[0], n[1], n[2], h, o.x, o.y, o.z, d.x, d.y, d.z, 0.0, t)) return true;
  }
  return false;
}

static Mesh tetrahedron() {
  Mesh m;
  m.v = {{1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}};
  m.f = {0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 2};
  return m;
}
static Mesh icosahedron() {
  const double t = (1.0 + std::sqrt(5.0)) / 2.0;
  Mesh m;
  m.v = {{-1, t, 0}, {1, t, 0}, {-1, -t, 0}, {1, -t, 0}, {0, -1, t}, {0, 1, t},
         {0, -1, -t}, {0, 1, -t}, {t, 0, -1}, {t, 0, 1}, {-t, 0, -1}, {-t, 0, 1}};
  m.f = {0, 11, 5, 0, 5, 1, 0, 1, 7, 0, 7, 10, 0, 10, 11, 1, 5, 9, 5, 11, 4, 11, 10, 2, 10, 7, 6, 7, 1, 8,
         3, 9, 4, 3, 4, 2, 3, 2, 6, 3, 6, 8, 3, 8, 9, 4, 9, 5, 2, 4, 11, 6, 2, 10, 8, 6, 7, 9, 8, 1};
  return m;
}
static Mesh subdivide(const Mesh& in) {  // each face into four; midpoints shared by index
  Mesh m;
  m.v = in.v;
  std::vector<std::pair<uint64_t, int>> mids;
  auto mid = [&](int a, int b) {
    const uint64_t key = a < b ? ((uint64_t)a << 32) | (uint32_t)b : ((uint64_t)b << 32) | (uint32_t)a;
    for (auto& e : mids)
      if (e.first == key) return e.second;
    const P3 &p = in.v[a], &q = in.v[b];
    P3 c{(p.x + q.x) / 2, (p.y + q.y) / 2, (p.z + q.z) / 2};
    const double l = std::sqrt(c.x * c.x + c.y * c.y + c.z * c.z);
    c = {c.x / l, c.y / l, c.z / l};
    m.v.push_back(c);
    mids.push_back({key, (int)m.v.size() - 1});
    return (int)m.v.size() - 1;
  };
  for (size_t i = 0; i + 2 < in.f.size(); i += 3) {
    const int a = in.f[i], b = in.f[i + 1], c = in.f[i + 2];
    const int ab = mid(a, b), bc = mid(b, c), ca = mid(c, a);
    const int add[12] = {a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca};
    m.f.insert(m.f.end(), add, add + 12);
  }
  return m;
}

int main() {
  std::mt19937_64 rng(20260);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  // ---- 1. axis-aligned triangles against the rect's statements
  for (int k = 0; k < 3; ++k) {
    const int ia = k == 0 ? 1 : 0, ib = k == 2 ? 1 : 2;  // the rect's in-plane axes (YZ: y, z; XZ: x, z; XY: x, y)
    for (int wind = 0; wind < 2; ++wind) {
      for (int rep = 0; rep < 20; ++rep) {
        const double kk = rep == 0 ? 0.0 : 300.0 * U(rng);
        double v[3][3];
        for (int c = 0; c < 3; ++c) v[c][k] = kk, v[c][ia] = 10.0 * U(rng), v[c][ib] = 10.0 * U(rng);
        double a[9], n[3], h;
        for (int c = 0; c < 3; ++c)
          for (int j = 0; j < 3; ++j) a[3 * c + j] = v[c][j];
        if (!rtwtri::derive(a, n, h)) continue;
        if (wind) {  // the other winding: exchange v1 and v2
          for (int j = 0; j < 3; ++j) std::swap(a[3 + j], a[6 + j]);
          CHECK(rtwtri::derive(a, n, h), "winding made it degenerate");
        }
        const double sgn = n[k] > 0 ? 1.0 : -1.0;
        for (int j = 0; j < 3; ++j)
          CHECK(bits(n[j]) == bits(j == k ? sgn : 0.0), "axis %d winding %d: n[%d] = %a", k, wind, j, n[j]);
        CHECK(bits(h) == bits(sgn * kk) || (kk == 0.0 && h == 0.0), "axis %d: h = %a for k = %a", k, h, kk);
        for (int r = 0; r < 900; ++r) {  // (3 axes x 2 windings x 20 planes x 900 rays = 108,000)
          double o[3] = {400.0 * U(rng), 400.0 * U(rng), 400.0 * U(rng)}, d[3] = {U(rng), U(rng), U(rng)};
          if (r % 50 == 0) d[(k + 1) % 3] = 0.0;
          if (d[k] == 0.0) continue;
          double t;
          const bool ok = rtwtri::plane_t(n[0], n[1], n[2], h, o[0], o[1], o[2], d[0], d[1], d[2], t);
          const double want = (kk - o[k]) / d[k];  // rect_root (rtw_world_walk.hpp)
          CHECK(ok && bits(t) == bits(want), "axis %d winding %d: t = %a, the rect's %a", k, wind, t, want);
          // the rect's hit record (hit_record): front = dot(e_k, d) < 0, normal e_k or e_k * -1
          double e[3] = {0.0, 0.0, 0.0};
          e[k] = 1.0;
          const bool rfront = e[0] * d[0] + e[1] * d[1] + e[2] * d[2] < 0.0;
          const bool tfront = n[0] * d[0] + n[1] * d[1] + n[2] * d[2] < 0.0;
          for (int j = 0; j < 3; ++j) {
            const double rn = rfront ? e[j] : e[j] * -1.0, tn = tfront ? n[j] : n[j] * -1.0;
            // n = +e_k: the rect's bits.  n = -e_k: the rect's values; the signs of the two zero components
            // are the opposite ones, since n keeps +0 zeros and the facing normal is n or -n.
            CHECK(sgn > 0 ? bits(rn) == bits(tn) : (rn == tn && (j == k || bits(rn) == (bits(tn) ^ (1ull << 63)))),
                  "axis %d winding %d: normal[%d] %a, the rect's %a", k, wind, j, tn, rn);
            CHECK(bits(o[j] + d[j] * t) == bits(o[j] + d[j] * want), "p[%d]", j);
          }
        }
      }
    }
  }
  // ---- 2. watertightness
  std::vector<Mesh> meshes = {tetrahedron(), icosahedron(), subdivide(subdivide(icosahedron()))};
  for (auto& p : meshes[2].v) p = {p.x * (1 + 0.05 * U(rng)) + 0.01 * U(rng), p.y * (1 + 0.05 * U(rng)), p.z * (1 + 0.05 * U(rng))};
  for (size_t mi = 0; mi < meshes.size(); ++mi) {
    const Mesh& m = meshes[mi];
    for (int oi = 0; oi < 3; ++oi) {
      const P3 o{0.11 * oi + 0.01 * U(rng), 0.07 * U(rng), -0.09 * oi};
      auto aim = [&](const P3& q, const char* what, size_t id) {
        for (int variant = 0; variant < 9; ++variant) {
          P3 d{q.x - o.x, q.y - o.y, q.z - o.z};
          if (variant) {  // a few ulps beside, in one component
            double* c = (variant - 1) % 3 == 0 ? &d.x : ((variant - 1) % 3 == 1 ? &d.y : &d.z);
            *c = step(*c, (variant - 1) / 3 == 0 ? 1 : ((variant - 1) / 3 == 1 ? -1 : 3));
          }
          const double sc = variant == 8 ? 0x1p-100 : (variant == 7 ? 0x1p100 : 1.0);
          d = {d.x * sc, d.y * sc, d.z * sc};
          CHECK(hits_any(m, o, d), "mesh %zu: a ray to %s %zu (variant %d) hits nothing", mi, what, id, variant);
        }
      };
      for (size_t i = 0; i < m.v.size(); ++i) aim(m.v[i], "vertex", i);
      for (size_t i = 0; i + 2 < m.f.size(); i += 3)
        for (int e = 0; e < 3; ++e) {
          const P3 &p = m.v[m.f[i + e]], &q = m.v[m.f[i + (e + 1) % 3]];
          for (double s : {0.5, 0.25, 0.0625, 0.9, 1.0 / 3.0}) aim({p.x + s * (q.x - p.x), p.y + s * (q.y - p.y), p.z + s * (q.z - p.z)}, "edge of face", i / 3);
        }
    }
  }
  for (int rep = 0; rep < 200; ++rep) {  // planar quads split along a diagonal (general planes and axis-aligned)
    P3 c{3 * U(rng), 3 * U(rng), 3 * U(rng)}, e1{U(rng), U(rng), U(rng)}, e2{U(rng), U(rng), U(rng)};
    if (rep % 4 == 0) e1 = {1.0 + U(rng) * 0.5, 0, 0}, e2 = {0, 0, 1.0 + 0.5 * U(rng)};
    Mesh q;
    q.v = {c, {c.x + e1.x, c.y + e1.y, c.z + e1.z}, {c.x + e1.x + e2.x, c.y + e1.y + e2.y, c.z + e1.z + e2.z}, {c.x + e2.x, c.y + e2.y, c.z + e2.z}};
    q.f = {0, 1, 2, 0, 2, 3};
    const P3 o{c.x + 5 * U(rng), c.y + 7.0, c.z + 5 * U(rng)};
    for (int r = 0; r < 60; ++r) {
      const double s = r < 20 ? r / 19.0 : 0.5 * (U(rng) + 1), w = r < 20 ? s : (r < 40 ? s : 0.5 * (U(rng) + 1));
      // r < 40: points on the diagonal (s == w); else anywhere in the quad
      P3 t{c.x + s * e1.x + w * e2.x, c.y + s * e1.y + w * e2.y, c.z + s * e1.z + w * e2.z};
      for (int ul = -2; ul <= 2; ++ul) {
        P3 d{step(t.x - o.x, ul), t.y - o.y, step(t.z - o.z, -ul)};
        double a[9] = {q.v[0].x, q.v[0].y, q.v[0].z, q.v[1].x, q.v[1].y, q.v[1].z, q.v[2].x, q.v[2].y, q.v[2].z}, n[3], h;
        if (!rtwtri::derive(a, n, h)) continue;
        if (s > 0.02 && s < 0.98 && w > 0.02 && w < 0.98)
          CHECK(hits_any(q, o, d), "quad %d: a ray through (%g, %g) misses both halves", rep, s, w);
      }
    }
  }
  // ---- 3. barycentrics: the bound of DESIGN.md §22
  double worst = 0.0;
  for (int rep = 0; rep < 200000; ++rep) {
    double a[9], n[3], h;
    const double sc = rep % 3 == 0 ? 1.0 : (rep % 3 == 1 ? 100.0 : 0.01);
    for (double& x : a) x = sc * 4.0 * U(rng);
    if (!rtwtri::derive(a, n, h)) continue;
    const double s = 0.5 * (U(rng) + 1), w = 0.5 * (U(rng) + 1) * (1 - s);
    const double tx = a[0] + s * (a[3] - a[0]) + w * (a[6] - a[0]), ty = a[1] + s * (a[4] - a[1]) + w * (a[7] - a[1]),
                 tz = a[2] + s * (a[5] - a[2]) + w * (a[8] - a[2]);
    const double o[3] = {sc * 6 * U(rng), sc * 6 * U(rng), sc * 6 * U(rng)};
    const double dsc = rep % 5 == 0 ? 0x1p40 : 1.0;
    const double d[3] = {(tx - o[0]) * dsc, (ty - o[1]) * dsc, (tz - o[2]) * dsc};
    double t;
    if (!rtwtri::root(a, n[0], n[1], n[2], h, o[0], o[1], o[2], d[0], d[1], d[2], 0.0, t)) continue;
    double bu, bv, w0, w1, w2;
    rtwtri::bary(a, o[0], o[1], o[2], d[0], d[1], d[2], bu, bv);
    rtwtri::edges(a, o[0], o[1], o[2], d[0], d[1], d[2], w0, w1, w2);
    double err = 0, L = 0, E = 0;
    for (int j = 0; j < 3; ++j) {
      const double p = o[j] + d[j] * t, q = a[j] + bu * (a[3 + j] - a[j]) + bv * (a[6 + j] - a[j]);
      err = std::fmax(err, std::fabs(p - q));
      for (int c = 0; c < 3; ++c) L = std::fmax(L, std::fabs(a[3 * c + j] - o[j])), L = std::fmax(L, std::fabs(a[3 * c + j]));
      L = std::fmax(L, std::fabs(o[j]));
      E = std::fmax(E, std::fmax(std::fabs(a[3 + j] - a[j]), std::fabs(a[6 + j] - a[j])));
    }
    L *= std::sqrt(3.0), E *= std::sqrt(3.0);
    const double dn = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), S = std::fabs(w0 + w1 + w2);
    const double nd = std::fabs(n[0] * d[0] + n[1] * d[1] + n[2] * d[2]);
    const double u = 0x1p-53;
    const double bound = 256.0 * u * dn * L * L * E / S + 16.0 * u * L * dn / nd + 8.0 * u * L;
    worst = std::fmax(worst, err / bound);
    CHECK(err <= bound, "barycentric point off by %g, bound %g (u %g v %g)", err, bound, bu, bv);
    CHECK(bu >= -1e-9 && bv >= -1e-9 && bu + bv <= 1 + 1e-9, "u %g v %g outside the triangle", bu, bv);
    double t0, t1, t2;  // edge_tau's value is edges' (the same operations)
    const double e0 = rtwtri::edge_tau(a[3] - o[0], a[4] - o[1], a[5] - o[2], a[6] - o[0], a[7] - o[1], a[8] - o[2], d[0], d[1], d[2], t0);
    const double e1 = rtwtri::edge_tau(a[6] - o[0], a[7] - o[1], a[8] - o[2], a[0] - o[0], a[1] - o[1], a[2] - o[2], d[0], d[1], d[2], t1);
    const double e1r = rtwtri::edge_tau(a[0] - o[0], a[1] - o[1], a[2] - o[2], a[6] - o[0], a[7] - o[1], a[8] - o[2], d[0], d[1], d[2], t2);
    CHECK(bits(e0) == bits(w0) && bits(e1) == bits(w1) && bits(e1r) == bits(-w1) && t1 == t2,
          "edge functions: %a %a, %a %a; antisymmetry %a %a", e0, w0, e1, w1, e1r, -w1);
  }
  // ---- 4. boxes through chains of 1-4 ops
  for (int rep = 0; rep < 20000; ++rep) {
    rtw_prim p;
    std::memset(&p, 0, sizeof(p));
    p.kind = RTW_PRIM_TRIANGLE;
    for (double& x : p.a) x = 50.0 * U(rng);
    rtw_xform xf;
    std::memset(&xf, 0, sizeof(xf));
    xf.n = 1 + rep % 4;
    uint32_t hdr = xf.n;
    double vals[12];
    for (uint32_t i = 0; i < xf.n; ++i) {
      xf.op[i] = (rep >> i) & 1;
      if (xf.op[i] == RTW_XF_TRANSLATE) {
        for (int c = 0; c < 3; ++c) xf.v[i][c] = 20.0 * U(rng);
      } else {
        const double t = 3.2 * U(rng);
        xf.v[i][0] = std::sin(t), xf.v[i][1] = std::cos(t), xf.v[i][2] = t;
      }
      hdr |= xf.op[i] << (8 + 4 * i);
      for (int c = 0; c < 3; ++c) vals[3 * i + c] = xf.v[i][c];
    }
    const Box b = prim_box(p, &xf);
    double lo[3], hi[3];
    rtwr::prim_box(5u, p.a, hdr, vals, lo, hi);
    CHECK(std::memcmp(lo, b.lo, 24) == 0 && std::memcmp(hi, b.hi, 24) == 0, "the two prim_box statements differ for a triangle");
    for (int c = 0; c < 3; ++c) {  // the vertex, object -> world (to_world's arithmetic)
      double q[3] = {p.a[3 * c], p.a[3 * c + 1], p.a[3 * c + 2]};
      for (int i = (int)xf.n - 1; i >= 0; --i) {
        if (xf.op[i] == RTW_XF_TRANSLATE) {
          for (int j = 0; j < 3; ++j) q[j] += xf.v[i][j];
        } else {
          const double sn = xf.v[i][0], cs = xf.v[i][1], x = q[0], z = q[2];
          q[0] = cs * x + sn * z, q[2] = -sn * x + cs * z;
        }
      }
      for (int j = 0; j < 3; ++j) CHECK(q[j] >= b.lo[j] && q[j] <= b.hi[j], "a vertex leaves the padded box on axis %d", j);
    }
  }
  // ---- 5. degenerate and non-finite triangles
  {
    double n[3], h;
    const double line[9] = {0, 0, 0, 1, 1, 1, 2, 2, 2}, point[9] = {1, 2, 3, 1, 2, 3, 1, 2, 3};
    double nan9[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, inf9[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, big[9] = {0, 0, 0, 1e200, 0, 0, 0, 1e200, 0};
    nan9[4] = NAN, inf9[8] = INFINITY;
    CHECK(!rtwtri::derive(line, n, h), "collinear vertices accepted");
    CHECK(!rtwtri::derive(point, n, h), "a point accepted");
    CHECK(!rtwtri::derive(nan9, n, h), "a NaN vertex accepted");
    CHECK(!rtwtri::derive(inf9, n, h), "an infinite vertex accepted");
    CHECK(!rtwtri::derive(big, n, h), "an overflowing area accepted");
    const double good[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
    CHECK(rtwtri::derive(good, n, h) && n[2] == 1.0, "a plain triangle refused");
    double t;
    CHECK(!rtwtri::root(good, n[0], n[1], n[2], h, 0.2, 0.2, 0.0, 1.0, 0.5, 0.0, 0.0, t), "an in-plane ray hits");
    // exact zeros are inside: straight down onto a vertex, and along an edge's plane (w == 0, tau == 0)
    CHECK(rtwtri::root(good, n[0], n[1], n[2], h, 0.0, 0.0, 3.0, 0.0, 0.0, -1.0, 0.0, t) && t == 3.0, "a ray onto v0 misses");
    CHECK(rtwtri::root(good, n[0], n[1], n[2], h, 1.0, 0.0, 3.0, 0.0, 0.0, -1.0, 0.0, t) && t == 3.0, "a ray onto v1 misses");
    CHECK(rtwtri::root(good, n[0], n[1], n[2], h, 0.5, 0.0, 2.0, 0.0, 0.0, -1.0, 0.0, t) && t == 2.0, "a ray onto the edge v0 v1 misses");
    CHECK(rtwtri::root(good, n[0], n[1], n[2], h, 0.5, 0.0, -2.0, 0.0, 0.0, 1.0, 0.0, t) && t == 2.0, "... from behind");
    CHECK(!rtwtri::root(good, n[0], n[1], n[2], h, 0.5, -0.001, 2.0, 0.0, 0.0, -1.0, 0.0, t), "a ray beside the edge hits");
  }
  printf("tri_check: checks %llu violations %llu bary_ratio %.4g\n", g_checks, g_viol, worst);
  return g_viol ? 1 : 0;
}
