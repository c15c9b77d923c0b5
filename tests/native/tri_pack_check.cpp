// tri_pack_check — triangles through the world packer, the refit and the rebuild's host twin
// (csrc/rtw_world_pack.cpp, rtw_world_refit.cpp, rtw_world_build.cpp) with a plain C++ compiler:
//   * a world with a triangle sets feature bit 64, a world without one does not and leaves doubles
//     12-13 of every record zero;
//   * a triangle's record holds its vertices, n (doubles 9, 10, 12) and h (13) as rtw_tri.hpp derives
//     them, and double 11 keeps the per-lane walk's {kind, list index};
//   * every node box holds the (chain-moved) vertices of the triangles below it;
//   * a degenerate or non-finite triangle is refused by the packer (RTW_EINVAL), by refit_world and by
//     rebuild_world, which leave the tables untouched;
//   * a refit with moved vertices leaves the records a fresh pack of those vertices has.
// Prints "tri_pack_check: checks N violations M"; exit status 1 on a violation.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "rtw_layout.hpp"
#include "rtw_tri.hpp"
#include "rtw_world_pack.hpp"

static unsigned long long g_checks = 0, g_viol = 0;
#define CHECK(c, ...)                   \
  do {                                  \
    ++g_checks;                         \
    if (!(c)) {                         \
      if (++g_viol <= 10) {             \
        fprintf(stderr, "VIOLATION: "); \
        fprintf(stderr, __VA_ARGS__);   \
        fprintf(stderr, "\n");          \
      }                                 \
    }                                   \
  } while (0)

struct World {
  std::vector<rtw_prim> prims;
  std::vector<rtw_xform> xf;
  rtw_texture tex;
  rtw_wmaterial mat;
  rtw_world_desc desc() {
    rtw_world_desc d;
    std::memset(&d, 0, sizeof(d));
    d.prims = prims.data(), d.n_prims = (uint32_t)prims.size();
    d.xforms = xf.data(), d.n_xforms = (uint32_t)xf.size();
    d.textures = &tex, d.n_textures = 1, d.mats = &mat, d.n_mats = 1;
    return d;
  }
};

static World make(int n_tris, int n_spheres, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  World w;
  std::memset(&w.tex, 0, sizeof(w.tex));
  std::memset(&w.mat, 0, sizeof(w.mat));
  w.tex.color[0] = w.tex.color[1] = w.tex.color[2] = 0.5;
  for (int c = 0; c < 4; ++c) {  // chains of 1-4 ops
    rtw_xform x;
    std::memset(&x, 0, sizeof(x));
    x.n = c + 1;
    for (uint32_t i = 0; i < x.n; ++i) {
      x.op[i] = (c + i) & 1;
      if (x.op[i] == RTW_XF_TRANSLATE) {
        for (int j = 0; j < 3; ++j) x.v[i][j] = 3.0 * U(rng);
      } else {
        const double t = 2.0 * U(rng);
        x.v[i][0] = std::sin(t), x.v[i][1] = std::cos(t), x.v[i][2] = t;
      }
    }
    w.xf.push_back(x);
  }
  const int total = n_tris + n_spheres;
  for (int i = 0; i < total; ++i) {
    rtw_prim p;
    std::memset(&p, 0, sizeof(p));
    const double c[3] = {20.0 * U(rng), 20.0 * U(rng), 20.0 * U(rng)};
    if ((i % 3 != 2 || n_spheres == 0) && n_tris > 0) {
      --n_tris;
      p.kind = RTW_PRIM_TRIANGLE;
      for (int k = 0; k < 9; ++k) p.a[k] = c[k % 3] + U(rng);
      p.xform = i % 3 == 0 ? (i / 3) % 4 : -1;
    } else {
      p.kind = RTW_PRIM_SPHERE;
      for (int k = 0; k < 3; ++k) p.a[k] = p.a[3 + k] = c[k];
      p.a[6] = 0.3 + 0.2 * U(rng);
      p.xform = -1;
    }
    w.prims.push_back(p);
  }
  return w;
}

static void to_world(const rtw_xform& xf, double q[3]) {
  for (int i = (int)xf.n - 1; i >= 0; --i) {
    if (xf.op[i] == RTW_XF_TRANSLATE) {
      for (int j = 0; j < 3; ++j) q[j] += xf.v[i][j];
    } else {
      const double sn = xf.v[i][0], cs = xf.v[i][1], x = q[0], z = q[2];
      q[0] = cs * x + sn * z, q[2] = -sn * x + cs * z;
    }
  }
}

static void check_records(World& w, const rtwp::WorldPack& k, const char* what) {
  const double* prim = reinterpret_cast<const double*>(k.blob.data() + k.o_prim);
  const uint32_t* order = reinterpret_cast<const uint32_t*>(k.blob.data() + k.o_order);
  for (uint32_t i = 0; i < k.n_prims; ++i) {
    const double* r = prim + (size_t)rtwk::kWorldRec * order[i];
    const rtw_prim& p = w.prims[i];
    uint32_t lane[2], meta[4];
    std::memcpy(lane, r + 11, 8), std::memcpy(meta, r + 14, 16);
    CHECK(lane[0] == meta[0] && lane[1] == i && meta[2] == i && (meta[0] & 0xFFu) == p.kind, "%s: prim %u: meta words", what, i);
    if (p.kind != RTW_PRIM_TRIANGLE) {
      CHECK(r[12] == 0.0 && r[13] == 0.0, "%s: prim %u: doubles 12-13 of a non-triangle", what, i);
      continue;
    }
    double n[3], h;
    CHECK(rtwtri::derive(p.a, n, h), "%s: prim %u is degenerate", what, i);
    const double want[13] = {p.a[0], p.a[1], p.a[2], p.a[3], p.a[4], p.a[5], p.a[6], p.a[7], p.a[8], n[0], n[1], n[2], h};
    const double got[13] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[12], r[13]};
    CHECK(std::memcmp(want, got, sizeof(want)) == 0, "%s: prim %u: the triangle's record", what, i);
  }
  // node boxes hold the vertices of the triangles below them (leaves only: interior boxes are unions)
  const float* node = reinterpret_cast<const float*>(k.blob.data() + k.o_node);
  for (uint32_t nd = 0; nd < k.n_nodes; ++nd)
    for (int c = 0; c < 2; ++c) {
      uint32_t ref;
      std::memcpy(&ref, node + (size_t)rtwk::kNodeWords * nd + 12 + c, 4);
      if (!(ref & rtwk::kLeafBit)) continue;
      const uint32_t first = ref & 0x7FFFFFu, cnt = (ref >> 23) & rtwk::kLeafCountMask;
      for (uint32_t pos = first; pos < first + cnt; ++pos) {
        uint32_t meta[4];
        std::memcpy(meta, prim + (size_t)rtwk::kWorldRec * pos + 14, 16);
        const rtw_prim& p = w.prims[meta[2]];
        if (p.kind != RTW_PRIM_TRIANGLE) continue;
        CHECK(!(ref & rtwk::kCullBit), "%s: a leaf with a triangle carries the pretest bit", what);
        for (int v = 0; v < 3; ++v) {
          double q[3] = {p.a[3 * v], p.a[3 * v + 1], p.a[3 * v + 2]};
          if (p.xform >= 0) to_world(w.xf[p.xform], q);
          const float* b = node + (size_t)rtwk::kNodeWords * nd;
          for (int j = 0; j < 3; ++j)
            CHECK(q[j] >= b[2 * j + c] && q[j] <= b[6 + 2 * j + c], "%s: a vertex of prim %u leaves its leaf box (axis %d)", what, meta[2], j);
        }
      }
    }
}

int main() {
  std::string msg;
  for (int size : {6, 40, 700}) {  // linear, leaves of two, leaves of one
    World w = make(size, size / 2, 11 + size);
    rtw_world_desc d = w.desc();
    rtwp::WorldPack k;
    CHECK(rtwp::pack_world(&d, 0, false, k, msg) == RTW_OK, "pack of %d triangles: %s", size, msg.c_str());
    CHECK((k.feat & 64u) != 0u && (k.feat & 8u) == 0u && (k.feat & 4u) != 0u, "feature bits 0x%x", k.feat);
    check_records(w, k, "pack");
    // refit with moved vertices == a fresh pack's records
    rtwp::RefitPack r;
    rtwp::make_refit(&d, k, r);
    World w2 = w;
    std::vector<double> a((size_t)9 * w.prims.size());
    for (size_t i = 0; i < w.prims.size(); ++i)
      for (int j = 0; j < 9; ++j) {
        w2.prims[i].a[j] = w.prims[i].a[j] + ((w.prims[i].kind == RTW_PRIM_TRIANGLE || j < 6) ? 0.01 * ((int)((i + j) % 5) - 2) : 0.0);
        if (w.prims[i].kind == RTW_PRIM_SPHERE && j >= 3 && j < 6) w2.prims[i].a[j] = w2.prims[i].a[j - 3];
        a[9 * i + j] = w2.prims[i].a[j];
      }
    const std::vector<unsigned char> before = k.blob;
    // a degenerate and a NaN triangle: refused, tables untouched
    for (int bad = 0; bad < 2; ++bad) {
      std::vector<double> ab = a;
      for (size_t i = 0; i < w.prims.size(); ++i)
        if (w.prims[i].kind == RTW_PRIM_TRIANGLE) {
          if (bad == 0)
            for (int j = 0; j < 3; ++j) ab[9 * i + 3 + j] = ab[9 * i + j], ab[9 * i + 6 + j] = ab[9 * i + j];
          else
            ab[9 * i + 7] = NAN;
          break;
        }
      CHECK(rtwp::refit_world(k, r, ab.data(), nullptr) == RTW_EINVAL && k.blob == before, "refit accepted a bad triangle (%d)", bad);
      if (rtwp::rebuild_supported(k.n_prims, k.n_nodes, k.info))
        CHECK(rtwp::rebuild_world(k, r, ab.data(), nullptr) == RTW_EINVAL && k.blob == before, "rebuild accepted a bad triangle (%d)", bad);
    }
    CHECK(rtwp::refit_world(k, r, a.data(), nullptr) == RTW_OK, "refit: %s", r.msg.c_str());
    check_records(w2, k, "refit");
    if (rtwp::rebuild_supported(k.n_prims, k.n_nodes, k.info)) {
      CHECK(rtwp::rebuild_world(k, r, a.data(), nullptr) == RTW_OK && rtwp::refit_world(k, r, a.data(), nullptr) == RTW_OK, "rebuild: %s", r.msg.c_str());
      check_records(w2, k, "rebuild");
    }
    // creation refuses the same
    for (int bad = 0; bad < 3; ++bad) {
      World wb = w;
      for (auto& p : wb.prims)
        if (p.kind == RTW_PRIM_TRIANGLE) {
          if (bad == 0)
            for (int j = 0; j < 3; ++j) p.a[3 + j] = p.a[j];  // v1 == v0: zero area
          else
            p.a[4] = bad == 1 ? NAN : INFINITY;
          break;
        }
      rtw_world_desc db = wb.desc();
      rtwp::WorldPack kb;
      CHECK(rtwp::pack_world(&db, 0, false, kb, msg) == RTW_EINVAL, "the packer accepted a bad triangle (%d)", bad);
    }
  }
  {  // a world without triangles: no bit, doubles 12-13 zero
    World w = make(0, 50, 3);
    rtw_world_desc d = w.desc();
    rtwp::WorldPack k;
    CHECK(rtwp::pack_world(&d, 0, false, k, msg) == RTW_OK && (k.feat & 64u) == 0u, "a sphere world: feature bits 0x%x", k.feat);
    check_records(w, k, "spheres");
  }
  printf("tri_pack_check: checks %llu violations %llu\n", g_checks, g_viol);
  return g_viol ? 1 : 0;
}
