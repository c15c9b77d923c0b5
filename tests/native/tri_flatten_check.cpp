// tri_flatten_check — the C++ mirror's triangle (csrc/rtw_host.hpp Hittable::makeTriangle) through
// flattenWorld (csrc/rtw_world_host.cpp): kind 5 with its three vertices in a[0..8], its material, and
// the enclosing Translate / RotateY wrappers as its chain (op 0 outermost); the flattened description
// then packs, and rtw_tri.hpp finds the triangle sound.
// Prints "tri_flatten_check: checks N violations M"; exit status 1 on a violation.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "rtw_host.hpp"
#include "rtw_tri.hpp"

// (rtw_host.cpp's rtw::render calls into the library, which this program does not link: never reached here)
extern "C" int rtw_render(const rtw_camera*, const rtw_sphere*, uint32_t, const rtw_material*, uint32_t, const rtw_params*,
                          uint8_t*, float*) {
  return RTW_UNSUPPORTED;
}
extern "C" const char* rtw_last_error(void) { return "not linked"; }

static unsigned long long g_checks = 0, g_viol = 0;
#define CHECK(c, ...)                   \
  do {                                  \
    ++g_checks;                         \
    if (!(c)) {                         \
      ++g_viol;                         \
      fprintf(stderr, "VIOLATION: ");   \
      fprintf(stderr, __VA_ARGS__);     \
      fprintf(stderr, "\n");            \
    }                                   \
  } while (0)

int main() {
  using namespace rtw;
  auto red = Material::diffuse(Texture::makeSolid(Color{0.7, 0.2, 0.2}));
  auto steel = Material::metal(Color{0.8, 0.8, 0.9}, 0.1);
  const Point3 v0{0.0, 0.0, 0.0}, v1{2.0, 0.0, 0.5}, v2{0.5, 1.5, 0.0};
  std::vector<Hittable> objs;
  objs.push_back(Hittable::makeSphere(Point3{0, -100, 0}, 100.0, red));
  objs.push_back(Hittable::makeTriangle(v0, v1, v2, steel));
  auto inner = std::make_shared<Hittable>(Hittable::makeTriangle(v2, v1, v0, red));
  auto rot = std::make_shared<Hittable>(Hittable::makeRotateY(inner, 0.4));
  objs.push_back(Hittable::makeTranslate(rot, Vec3{1.0, 2.0, 3.0}));
  const FlatWorld f = flattenWorld(Hittable::makeList(objs));
  CHECK(f.prims.size() == 3, "%zu primitives", f.prims.size());
  if (f.prims.size() == 3) {
    const rtw_prim &a = f.prims[1], &b = f.prims[2];
    CHECK(f.prims[0].kind == RTW_PRIM_SPHERE && a.kind == RTW_PRIM_TRIANGLE && b.kind == RTW_PRIM_TRIANGLE, "kinds %u %u %u",
          f.prims[0].kind, a.kind, b.kind);
    const double want_a[9] = {0.0, 0.0, 0.0, 2.0, 0.0, 0.5, 0.5, 1.5, 0.0}, want_b[9] = {0.5, 1.5, 0.0, 2.0, 0.0, 0.5, 0.0, 0.0, 0.0};
    for (int k = 0; k < 9; ++k) CHECK(a.a[k] == want_a[k] && b.a[k] == want_b[k], "vertex number %d: %g %g", k, a.a[k], b.a[k]);
    CHECK(a.xform == -1 && b.xform >= 0 && (size_t)b.xform < f.xforms.size(), "chains %d %d", a.xform, b.xform);
    CHECK(a.mat != b.mat && b.mat == f.prims[0].mat, "materials %u %u %u", f.prims[0].mat, a.mat, b.mat);
    CHECK(a.mat < f.materials.size() && f.materials[a.mat].kind == RTW_WMAT_METAL, "the triangle's material");
    if (b.xform >= 0 && (size_t)b.xform < f.xforms.size()) {
      const rtw_xform& x = f.xforms[b.xform];
      CHECK(x.n == 2 && x.op[0] == RTW_XF_TRANSLATE && x.op[1] == RTW_XF_ROTATE_Y, "chain of %u ops: %u %u", x.n, x.op[0], x.op[1]);
      CHECK(x.v[0][0] == 1.0 && x.v[0][1] == 2.0 && x.v[0][2] == 3.0 && x.v[1][0] == std::sin(0.4) && x.v[1][1] == std::cos(0.4),
            "chain values");
    }
    double n[3], h, m[3], g;
    CHECK(rtwtri::derive(a.a, n, h) && rtwtri::derive(b.a, m, g), "a flattened triangle is degenerate");
    for (int k = 0; k < 3; ++k) CHECK(n[k] == -m[k], "the reversed winding's normal, component %d", k);
  }
  const rtw_world_desc d = f.desc();
  CHECK(d.n_prims == 3 && d.prims[1].kind == RTW_PRIM_TRIANGLE, "the description");
  printf("tri_flatten_check: checks %llu violations %llu\n", g_checks, g_viol);
  return g_viol ? 1 : 0;
}
