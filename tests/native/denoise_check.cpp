// denoise_check.cpp — properties of the denoiser's filter (csrc/rtw_denoise.hpp)
// with a plain C++ compiler, no HIP and no library: the level loop below is the
// one rtw_denoise_host runs.  tests/test_denoise_cpu.py builds and runs it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rtw_denoise.hpp"

using rtwd::Guide;
using rtwd::Px;

static int g_bad = 0, g_checks = 0;
#define CHECK(cond, ...)            \
  do {                              \
    ++g_checks;                     \
    if (!(cond)) {                  \
      ++g_bad;                      \
      std::printf("FAIL %s:%d ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);     \
      std::printf("\n");            \
    }                               \
  } while (0)

static std::vector<Px> run(std::vector<Px> img, const std::vector<Guide>* guides, int W, int H, uint32_t levels,
                           uint32_t flags = 0) {
  rtwd::Params P;
  if (!rtwd::resolve(levels, 0, 0, 0, 0, flags, P)) {
    CHECK(false, "resolve refused levels %u", levels);
    return img;
  }
  std::vector<Px> out(img.size());
  for (uint32_t l = 0; l < P.levels; ++l) {
    auto px = [&](int x, int y) { return img[(size_t)y * W + x]; };
    auto gd = [&](int x, int y) { return (*guides)[(size_t)y * W + x]; };
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x)
        out[(size_t)y * W + x] = guides ? rtwd::filter_pixel<true>(x, y, W, H, 1 << l, P, px, gd)
                                        : rtwd::filter_pixel<false>(x, y, W, H, 1 << l, P, px, gd);
    img.swap(out);
  }
  return img;
}

static Guide hit_guide(float depth, uint32_t prim) {
  Guide g{};
  g.n[2] = 1.0f;
  g.depth = depth;
  g.albedo[0] = g.albedo[1] = g.albedo[2] = 0.5f;
  g.prim = prim;
  return g;
}

static float ulps(float a, float b) { return std::fabs(a - b) / (std::fabs(b) * 1.1920929e-7f); }

// A deterministic value in [0, 1).
static float noise(uint32_t i) {
  i = i * 747796405u + 2891336453u;
  i = ((i >> ((i >> 28) + 4u)) ^ i) * 277803737u;
  return (float)((i >> 22) ^ i) / 4294967296.0f;
}

int main() {
  // 1. A constant image comes back constant within a few f32 ulp (guided or
  //    not, known or unknown variance, every number of levels).
  for (int guided = 0; guided < 2; ++guided)
    for (float var : {0.0f, 0.01f, rtwd::kVarUnknown})
      for (uint32_t levels = 1; levels <= rtwd::kMaxLevels; ++levels) {
        const int W = 37, H = 21;
        std::vector<Px> img((size_t)W * H, Px{0.3f, 0.6f, 0.1f, var});
        std::vector<Guide> g((size_t)W * H, hit_guide(3.0f, 1));
        const auto o = run(img, guided ? &g : nullptr, W, H, levels);
        float worst = 0.0f;
        for (const Px& p : o) worst = std::fmax(worst, std::fmax(ulps(p.r, 0.3f), std::fmax(ulps(p.g, 0.6f), ulps(p.b, 0.1f))));
        CHECK(worst <= 4.0f, "constant image: %g ulp (guided %d var %g levels %u)", worst, guided, var, levels);
      }
  // 2. A step edge whose sides differ in prim (hit vs miss) is preserved: no
  //    value leaks across it, although the colour term alone (unknown
  //    variance) would blur it.
  {
    const int W = 40, H = 24;
    std::vector<Px> img((size_t)W * H);
    std::vector<Guide> g((size_t)W * H);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const bool left = x < 17;
        const float n = 0.05f * noise((uint32_t)(y * W + x));
        img[(size_t)y * W + x] = left ? Px{0.8f + n, 0.8f + n, 0.8f + n, rtwd::kVarUnknown} : Px{0.1f + n, 0.1f + n, 0.1f + n, rtwd::kVarUnknown};
        Guide m{};
        m.albedo[0] = m.albedo[1] = m.albedo[2] = 0.5f;
        g[(size_t)y * W + x] = left ? hit_guide(2.0f, 3) : m;
      }
    const auto o = run(img, &g, W, H, 5);
    bool ok = true, smoother = true;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const float v = o[(size_t)y * W + x].r;
        ok = ok && (x < 17 ? (v >= 0.8f && v <= 0.85f) : (v >= 0.1f && v <= 0.15f));  // within its own side's range
      }
    CHECK(ok, "hit/miss edge: a value left its side's range");
    // ... and the sides themselves were filtered (the noise shrank)
    float dev_in = 0.0f, dev_out = 0.0f;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < 17; ++x) {
        dev_in = std::fmax(dev_in, std::fabs(img[(size_t)y * W + x].r - 0.825f));
        dev_out = std::fmax(dev_out, std::fabs(o[(size_t)y * W + x].r - 0.825f));
      }
    smoother = dev_out < 0.5f * dev_in;
    CHECK(smoother, "hit/miss edge: the side was not filtered (%g -> %g)", dev_in, dev_out);
    const auto blurred = run(img, nullptr, W, H, 5);
    CHECK(blurred[(size_t)10 * W + 17].r > 0.2f, "the unguided filter was expected to blur the edge");
  }
  // 3. Taps outside the image are dropped: 1x1 and 5x3 images work.
  {
    const auto o = run({Px{0.25f, 0.5f, 0.75f, 0.01f}}, nullptr, 1, 1, 6);
    CHECK(o[0].r == 0.25f && o[0].g == 0.5f && o[0].b == 0.75f, "1x1: %g %g %g", o[0].r, o[0].g, o[0].b);
    CHECK(ulps(o[0].var, 0.01f) <= 4.0f, "1x1 variance: %g", o[0].var);
    std::vector<Px> img(15, Px{0.4f, 0.4f, 0.4f, 0.0f});
    std::vector<Guide> g(15, hit_guide(1.0f, 2));
    for (uint32_t levels = 1; levels <= 6; ++levels) {
      const auto p = run(img, &g, 5, 3, levels);
      float worst = 0.0f;
      for (const Px& q : p) worst = std::fmax(worst, ulps(q.r, 0.4f));
      CHECK(worst <= 4.0f, "5x3 levels %u: %g ulp", levels, worst);
    }
  }
  // 4. A zero-sample pixel stays 0 and does not darken its neighbours.
  {
    const int W = 20, H = 12;
    std::vector<Px> img((size_t)W * H, Px{0.5f, 0.5f, 0.5f, 0.02f});
    for (int i : {45, 46, 47, 66, 130}) img[i] = Px{0.0f, 0.0f, 0.0f, rtwd::kVarEmpty};
    const auto o = run(img, nullptr, W, H, 5);
    float worst = 0.0f;
    for (size_t i = 0; i < o.size(); ++i) {
      if (img[i].var == rtwd::kVarEmpty)
        CHECK(o[i].r == 0.0f && o[i].g == 0.0f && o[i].b == 0.0f && o[i].var == rtwd::kVarEmpty, "empty pixel %zu changed", i);
      else
        worst = std::fmax(worst, ulps(o[i].r, 0.5f));
    }
    CHECK(worst <= 4.0f, "neighbours of empty pixels: %g ulp from 0.5", worst);
  }
  // 5. Unknown variance = the colour term off, bit for bit (the colour).
  {
    const int W = 33, H = 19;
    std::vector<Px> a((size_t)W * H), b((size_t)W * H);
    std::vector<Guide> g((size_t)W * H);
    for (int i = 0; i < W * H; ++i) {
      const float r = noise(3u * i), gg = noise(3u * i + 1u), bb = noise(3u * i + 2u);
      a[i] = Px{r, gg, bb, rtwd::kVarUnknown};
      b[i] = Px{r, gg, bb, 0.001f + 0.01f * noise(7u * i)};
      g[i] = hit_guide(2.0f + noise(11u * i), 1u + (uint32_t)(i % 3));
      g[i].albedo[0] = 0.5f + 0.05f * noise(13u * i);
    }
    for (int guided = 0; guided < 2; ++guided) {
      const auto oa = run(a, guided ? &g : nullptr, W, H, 5);
      const auto ob = run(b, guided ? &g : nullptr, W, H, 5, rtwd::kFlagNoColor);
      const auto oc = run(b, guided ? &g : nullptr, W, H, 5);
      int diff = 0, diff_c = 0;
      for (int i = 0; i < W * H; ++i) {
        diff += std::memcmp(&oa[i], &ob[i], 12) != 0;
        diff_c += std::memcmp(&oa[i], &oc[i], 12) != 0;
      }
      CHECK(diff == 0, "unknown variance vs colour term off: %d pixels differ (guided %d)", diff, guided);
      CHECK(diff_c > 0, "the colour term changed nothing (guided %d): the comparison shows nothing", guided);
    }
  }
  // 6. Options out of range are refused.
  {
    rtwd::Params P;
    CHECK(!rtwd::resolve(7, 0, 0, 0, 0, 0, P), "levels 7 accepted");
    CHECK(!rtwd::resolve(0, -1.0, 0, 0, 0, 0, P), "negative sigma accepted");
    CHECK(!rtwd::resolve(0, 0, 0, 0, 0, 8u, P), "unknown flag accepted");
    CHECK(rtwd::resolve(0, 0, 0, 0, 0, 0, P) && P.levels == 5, "defaults");
  }
  std::printf("denoise_check: bad %d/%d\n", g_bad, g_checks);
  return g_bad ? 1 : 0;
}
