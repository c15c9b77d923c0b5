// Inputs of scene_pack_check.cpp and world_pack_check.cpp that no scene
// builder of the library makes: a generated cover-style scene with spheres of
// every table group in several time groups, and a procedural RGBA image.
#pragma once
#include <cstdint>
#include <vector>

#include "rtw_hip.h"

// The library's host side (rtw_host.cpp) calls these two; the checks never render.
extern "C" int rtw_render(const rtw_camera*, const rtw_sphere*, uint32_t, const rtw_material*, uint32_t,
                          const rtw_params*, uint8_t*, float*) {
  return RTW_ENODEV;
}
extern "C" const char* rtw_last_error(void) { return "stub"; }

namespace pack_inputs {

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uni() { return (double)(next() >> 11) * 0x1p-53; }  // [0, 1)
};

inline std::vector<rtw_material> five_materials() {
  std::vector<rtw_material> m(5);
  m[0].kind = RTW_LAMBERT_CHECKER;
  m[1].kind = RTW_LAMBERT_SOLID;
  m[2].kind = RTW_METAL, m[2].fuzz = 0.2;
  m[3].kind = RTW_DIELECTRIC, m[3].ir = 1.5;
  m[4].kind = RTW_LAMBERT_SOLID;
  const double alb[5][3] = {{0.9, 0.9, 0.9}, {0.6, 0.3, 0.2}, {0.8, 0.8, 0.7}, {1, 1, 1}, {0.2, 0.5, 0.8}};
  for (int i = 0; i < 5; ++i)
    for (int k = 0; k < 3; ++k) m[i].albedo[k] = alb[i][k];
  m[0].albedo_odd[0] = 0.2, m[0].albedo_odd[1] = 0.3, m[0].albedo_odd[2] = 0.1;
  return m;
}

// n_narrow narrow spheres in the shape of tests/test_gpu_parity.py
// clustered_scene: every fourth static, the others movers along x, along y
// only and along z, in three time groups; with `wide`, a static and a moving
// sphere of radius >= 100 (the second ahead of every narrow mover, so the
// narrow movers' time groups are not all group 0).  `movers_only`: no static
// narrow sphere.
inline std::vector<rtw_sphere> generated_scene(uint32_t n_narrow, bool wide, uint64_t seed, bool movers_only = false) {
  const double groups[3][2] = {{0.0, 1.0}, {-0.5, 1.5}, {-1.0, 2.0}};
  Rng rng{seed};
  std::vector<rtw_sphere> out;
  auto sphere = [](double x, double y, double z, double r, uint32_t mat) {
    rtw_sphere s{};
    s.c0[0] = s.c1[0] = x, s.c0[1] = s.c1[1] = y, s.c0[2] = s.c1[2] = z;
    s.radius = r, s.mat = mat;
    return s;
  };
  if (wide) out.push_back(sphere(0, -1000, 0, 1000.0, 0));
  for (uint32_t k = 0; k < n_narrow; ++k) {
    if (wide && k == 1) {  // a moving wide sphere, far below the others; the list's first mover: it opens time group 0
      rtw_sphere s = sphere(3, -400, -2, 150.0, 1);
      s.c1[0] += 0.5, s.moving = 1, s.t0 = groups[2][0], s.t1 = groups[2][1];
      out.push_back(s);
    }
    const double x = -6 + 12 * rng.uni(), z = -6 + 12 * rng.uni(), r = 0.12 + 0.25 * rng.uni();
    rtw_sphere s = sphere(x, r, z, r, 1 + k % 4);
    const uint32_t kind = movers_only ? 1 + k % 3 : k % 4;  // 0 static, 1 x mover, 2 y mover, 3 z mover
    if (kind) {
      s.c1[kind - 1] += 0.2 + 0.4 * rng.uni();
      s.moving = 1, s.t0 = groups[k % 3][0], s.t1 = groups[k % 3][1];
    }
    out.push_back(s);
  }
  return out;
}

// A w x h RGBA8 image: smooth gradients with a checker on top.
inline std::vector<uint8_t> procedural_image(uint32_t w, uint32_t h) {
  std::vector<uint8_t> px((size_t)w * h * 4);
  for (uint32_t y = 0; y < h; ++y)
    for (uint32_t x = 0; x < w; ++x) {
      uint8_t* p = &px[((size_t)y * w + x) * 4];
      const bool chk = ((x / 4) ^ (y / 4)) & 1;
      p[0] = (uint8_t)(x * 255 / (w - 1)), p[1] = (uint8_t)(y * 255 / (h - 1)), p[2] = chk ? 200 : 40, p[3] = 255;
    }
  return px;
}

}  // namespace pack_inputs
