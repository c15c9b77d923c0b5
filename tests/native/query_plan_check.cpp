// query_plan_check.cpp — the host side of a ray query (csrc/rtw_query_plan.cpp):
// argument checks, the traversal after AUTO and the world's limits, the launch
// geometry, and rtw_pixel_ray's argument checks.  A stand-alone program, built
// with a plain C++ compiler and no HIP (tests/test_query_plan_host.py).
// Prints "checks N violations M"; exit status 1 when M > 0.
#include <cstdint>
#include <cstdio>
#include <string>

#include "rtw_query_plan.hpp"

static unsigned long long g_checks = 0, g_viol = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    ++g_checks;                                                         \
    if (!(cond)) {                                                      \
      ++g_viol;                                                         \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
    }                                                                   \
  } while (0)

int main() {
  std::string msg;
  alignas(16) static unsigned char buf[256];
  const void* h = buf;  // any non-null handle
  // ---- argument checks
  CHECK(rtwq::check_batch("t", h, buf, 5, nullptr, buf + 80, 8, msg) == RTW_OK);
  CHECK(rtwq::check_batch("t", nullptr, buf, 5, nullptr, buf, 8, msg) == RTW_EINVAL && !msg.empty());
  CHECK(rtwq::check_batch("t", h, nullptr, 5, nullptr, buf, 8, msg) == RTW_EINVAL);
  CHECK(rtwq::check_batch("t", h, buf, 5, nullptr, nullptr, 8, msg) == RTW_EINVAL);
  for (int off = 1; off < 8; ++off) {
    CHECK(rtwq::check_batch("t", h, buf + off, 5, nullptr, buf, 8, msg) == RTW_EINVAL);      // misaligned rays
    CHECK(rtwq::check_batch("t", h, buf, 5, nullptr, buf + off, 8, msg) == RTW_EINVAL);      // misaligned records
    CHECK(rtwq::check_batch("t", h, buf, 5, nullptr, buf + off, 1, msg) == RTW_OK);          // occlusion bytes: any
  }
  CHECK(rtwq::check_batch("t", h, buf + 8, 5, nullptr, buf + 24, 8, msg) == RTW_OK);  // 8-byte, not 16-byte, aligned
  // null pointers are refused before n is looked at; n == 0 itself is fine
  CHECK(rtwq::check_batch("t", h, buf, 0, nullptr, buf, 8, msg) == RTW_OK);
  CHECK(rtwq::check_batch("t", h, nullptr, 0, nullptr, buf, 8, msg) == RTW_EINVAL);
  // the n limit: 2^31 rays pass, one more does not
  CHECK(rtwq::check_batch("t", h, buf, RTW_QUERY_MAX_RAYS, nullptr, buf, 8, msg) == RTW_OK);
  CHECK(rtwq::check_batch("t", h, buf, RTW_QUERY_MAX_RAYS + 1, nullptr, buf, 8, msg) == RTW_EINVAL);
  CHECK(rtwq::check_batch("t", h, buf, ~0ull, nullptr, buf, 8, msg) == RTW_EINVAL);
  CHECK((uint64_t)(uint32_t)RTW_QUERY_MAX_RAYS == RTW_QUERY_MAX_RAYS);  // the kernels' 32-bit count holds it
  // options
  rtw_query_opts o = {0, 0};
  for (uint32_t t = 0; t <= 5; ++t) {
    o.traversal = t;
    CHECK((rtwq::check_batch("t", h, buf, 1, &o, buf, 8, msg) == RTW_OK) == (t <= RTW_WORLD_TRAVERSAL_LANE));
  }
  o.traversal = 0, o.flags = 1;
  CHECK(rtwq::check_batch("t", h, buf, 1, &o, buf, 8, msg) == RTW_EINVAL);

  // ---- traversal: LINEAR without a BVH whatever is asked; LANE only where the world allows it
  const uint32_t A = RTW_WORLD_TRAVERSAL_AUTO, U = RTW_WORLD_TRAVERSAL_UNION, L = RTW_WORLD_TRAVERSAL_LANE,
                 LIN = RTW_WORLD_TRAVERSAL_LINEAR;
  for (uint32_t asked : {A, U, L})
    for (bool ok : {false, true}) CHECK(rtwq::traversal(asked, 0, ok) == LIN);
  for (uint32_t nodes : {1u, 23u, RTW_QUERY_LANE_NODES - 1u, RTW_QUERY_LANE_NODES, 5802u}) {
    CHECK(rtwq::traversal(U, nodes, true) == U && rtwq::traversal(U, nodes, false) == U);
    CHECK(rtwq::traversal(L, nodes, true) == L && rtwq::traversal(L, nodes, false) == U);
    CHECK(rtwq::traversal(A, nodes, false) == U);
    CHECK(rtwq::traversal(A, nodes, true) == (nodes >= RTW_QUERY_LANE_NODES ? L : U));
  }

  // ---- launch geometry: ceil(n / 256) workgroups up to the resident ones, never 0
  const uint32_t cus = 256;
  for (uint32_t bpc : {1u, 4u, 5u}) {
    const uint32_t cap = cus * bpc;
    CHECK(rtwq::grid(0, cus, bpc) == 1);  // (n == 0 launches nothing: the entries return first)
    for (uint64_t n : {1ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 1000ull, 810000ull, (unsigned long long)cap * 256,
                       (unsigned long long)cap * 256 + 1, (unsigned long long)RTW_QUERY_MAX_RAYS}) {
      const uint32_t g = rtwq::grid(n, cus, bpc);
      CHECK(g >= 1 && g <= cap);
      const uint64_t want = (n + 255) / 256;
      CHECK(g == (want < cap ? (uint32_t)want : cap));
      // every ray has a lane on the first stride, or the grid is full and the kernels stride
      CHECK((uint64_t)g * rtwq::kBlock >= n || g == cap);
      // the per-lane kernel's ray index of wave w, k-th ray: (w + (k >> 6) * waves) * 64 + (k & 63) — the last
      // block any wave looks at lies below ceil(n / 64) + waves, whose 64-fold fits 32 bits
      const uint64_t waves = (uint64_t)g * (rtwq::kBlock / rtwq::kWaveRays);
      CHECK(((n + 63) / 64 + waves) * 64 < (1ull << 32));
    }
    CHECK(rtwq::grid(1, 0, bpc) == 1);  // an unknown CU count still launches
  }
  CHECK(rtwq::kBlock % rtwq::kWaveRays == 0);

  // ---- rtw_pixel_ray's argument checks (its values: tests/test_query_cpu.py)
  rtw_camera cam = {};
  rtw_ray r;
  CHECK(rtw_pixel_ray(&cam, 24, 14, 23, 13, &r) == RTW_OK && r.t_min == 0.001 && r.t_max > 1e308);
  CHECK(rtw_pixel_ray(nullptr, 24, 14, 0, 0, &r) == RTW_EINVAL);
  CHECK(rtw_pixel_ray(&cam, 24, 14, 0, 0, nullptr) == RTW_EINVAL);
  CHECK(rtw_pixel_ray(&cam, 24, 14, 24, 0, &r) == RTW_EINVAL);
  CHECK(rtw_pixel_ray(&cam, 24, 14, 0, 14, &r) == RTW_EINVAL);
  CHECK(rtw_pixel_ray(&cam, 1, 14, 0, 0, &r) == RTW_EINVAL);
  CHECK(rtw_pixel_ray(&cam, 24, 1, 0, 0, &r) == RTW_EINVAL);

  std::printf("checks %llu violations %llu\n", g_checks, g_viol);
  return g_viol ? 1 : 0;
}
