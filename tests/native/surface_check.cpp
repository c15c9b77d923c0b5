// surface_check.cpp — the argument check of the surface queries (csrc/rtw_surface.hpp
// check_call: what rtw_world_surface_device and rtw_scene_surface_device refuse) on the
// CPU, with no HIP: every listed refusal, what is NOT refused, and the byte-range
// overlap test against a brute-force statement of it over small ranges.  A plain
// program with its own main, so it also runs under the host sanitizers
// (tests/test_surface_cpu.py).  Prints "surface_check: bad B/N"; exit status 1 when B > 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "rtw_surface.hpp"

static int g_bad = 0, g_n = 0;
static void expect(bool ok, const char* what) {
  ++g_n;
  if (!ok) {
    ++g_bad;
    std::printf("FAIL %s\n", what);
  }
}

int main() {
  const uint64_t n = 37;
  // one arena, 16-byte aligned: hits | surf | guides, with room to slide the outputs over the hits
  std::vector<unsigned char> arena(64 + n * (80 + 64 + 32) + 256);
  unsigned char* base = arena.data() + ((16 - ((uintptr_t)arena.data() & 15u)) & 15u);
  unsigned char *hits = base, *surf = base + n * 80, *guides = surf + n * 64;
  const double bg[3] = {0.7, 0.8, 1.0};
  const double nan_bg[3] = {0.7, std::nan(""), 1.0}, inf_bg[3] = {std::numeric_limits<double>::infinity(), 0.8, 1.0};
  std::string msg;
  bool launch = true;
  auto call = [&](const void* h, uint64_t k, const double* b, const void* s, const void* g) {
    msg.clear();
    return rtws::check_call("surface_check", h, k, b, s, g, &launch, msg);
  };
  // accepted
  expect(call(hits, n, bg, surf, guides) == RTW_OK && launch, "both outputs");
  expect(call(hits, n, nullptr, surf, nullptr) == RTW_OK && launch, "surface only, no background");
  expect(call(hits, n, nan_bg, surf, nullptr) == RTW_OK && launch, "surface only ignores the background");
  expect(call(hits, n, bg, nullptr, guides) == RTW_OK && launch, "guides only");
  expect(call(nullptr, 0, nullptr, nullptr, nullptr) == RTW_OK && !launch, "n == 0 with null buffers launches nothing");
  expect(call(hits, RTW_QUERY_MAX_RAYS, nullptr, (void*)(uintptr_t)(1ull << 60), nullptr) == RTW_OK, "n == 2^31 is in range");
  expect(call(hits + 8, n, bg, hits + 8 + n * 80, nullptr) == RTW_OK, "8-byte aligned, adjacent ranges");
  // refused, each with a message and no launch
  struct Bad {
    const void* h;
    uint64_t k;
    const double* b;
    const void *s, *g;
    const char* what;
  } bad[] = {
      {nullptr, n, bg, surf, guides, "null d_hits"},
      {hits, n, bg, nullptr, nullptr, "both outputs null"},
      {hits, n, nullptr, surf, guides, "guides without a background"},
      {hits, n, nan_bg, surf, guides, "NaN background"},
      {hits, n, inf_bg, nullptr, guides, "infinite background"},
      {hits + 4, n, bg, surf, guides, "d_hits not 8-byte aligned"},
      {hits, n, bg, surf + 4, guides, "d_surf not 8-byte aligned"},
      {hits, n, bg, surf, guides + 8, "d_guides not 16-byte aligned"},
      {hits, RTW_QUERY_MAX_RAYS + 1, bg, surf, guides, "n > 2^31"},
      {hits, ~0ull, bg, surf, guides, "n = 2^64 - 1"},
      {hits, n, bg, hits, guides, "d_surf on d_hits"},
      {hits, n, bg, hits + n * 80 - 8, guides, "d_surf over the last word of d_hits"},
      {hits + 64 * n - 8, n, bg, hits, guides, "d_hits over the last word of d_surf"},
      {hits, n, bg, surf, hits + 16, "d_guides inside d_hits"},
      {hits, n, bg, surf, surf + 64 * n - 16, "d_guides over the end of d_surf"},
  };
  for (const Bad& b : bad) {
    const int st = call(b.h, b.k, b.b, b.s, b.g);
    expect(st == RTW_EINVAL && !launch && !msg.empty(), b.what);
  }
  // ranges_overlap against the definition: two ranges share a byte
  for (uint64_t a = 1; a < 12; ++a)
    for (uint64_t na = 0; na < 6; ++na)
      for (uint64_t b = 1; b < 12; ++b)
        for (uint64_t nb = 0; nb < 6; ++nb) {
          bool share = false;
          for (uint64_t x = a; x < a + na; ++x) share = share || (x >= b && x < b + nb);
          expect(rtws::ranges_overlap((const void*)(uintptr_t)a, na, (const void*)(uintptr_t)b, nb) == share, "ranges_overlap");
        }
  expect(!rtws::ranges_overlap(nullptr, 8, hits, 8) && !rtws::ranges_overlap(hits, 8, nullptr, 8), "a null range overlaps nothing");
  std::printf("surface_check: bad %d/%d\n", g_bad, g_n);
  return g_bad ? 1 : 0;
}
