// denoise_spatial_check.cpp — properties of the spatial variance estimate
// (csrc/rtw_denoise.hpp spatial_variance_pixel) with a plain
// C++ compiler, no HIP and no library: the image loop below is the one
// rtw_denoise_spatial_variance_host runs.  tests/test_denoise_spatial_cpu.py
// builds and runs it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rtw_denoise.hpp"

using rtwd::Guide;
using rtwd::kVarEmpty;
using rtwd::kVarUnknown;
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

static std::vector<float> estimate(const std::vector<Px>& img, const std::vector<Guide>* guides, int W, int H) {
  rtwd::Params P;
  if (!rtwd::resolve(0, 0, 0, 0, 0, rtwd::kFlagSpatialVar, P)) CHECK(false, "resolve refused the flag");
  std::vector<float> out(img.size());
  auto tap = [&](int x, int y) { return rtwd::sv_tap(img[(size_t)y * W + x]); };
  auto gd = [&](int x, int y) { return (*guides)[(size_t)y * W + x]; };
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const float vp = img[(size_t)y * W + x].var;
      out[(size_t)y * W + x] = guides ? rtwd::spatial_variance_pixel<true>(x, y, W, H, P, vp, tap, gd)
                                      : rtwd::spatial_variance_pixel<false>(x, y, W, H, P, vp, tap, gd);
    }
  return out;
}

static Guide hit_guide(float depth, uint32_t prim) {
  Guide g{};
  g.n[2] = 1.0f;
  g.depth = depth;
  g.albedo[0] = g.albedo[1] = g.albedo[2] = 0.5f;
  g.prim = prim;
  return g;
}

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// A deterministic value in [0, 1).
static float noise(uint32_t i) {
  i = i * 747796405u + 2891336453u;
  i = ((i >> ((i >> 28) + 4u)) ^ i) * 277803737u;
  return (float)((i >> 22) ^ i) / 4294967296.0f;
}

int main() {
  // 1. A constant image: variance exactly 0 everywhere (every pixel of a 9 x 6
  //    image keeps at least 4 taps), with and without guides.  Exactly 0 needs
  //    the window's sums to be exact — up to 49 Y and 49 Y^2 — which they are
  //    for a luminance of few significant bits: grey pixels c = k / 2^n, whose
  //    luminance is c itself (checked).  Any other constant is 0 within the
  //    rounding of those sums: s2/sw and m1^2 each carry a relative error of
  //    at most ~50 * 2^-53 (49 additions, a division, a product), so the
  //    difference is below 2^-46 Y^2 — eleven orders of magnitude under the
  //    colour scale's floor kEpsColor^2.
  for (int guided = 0; guided < 2; ++guided) {
    const int W = 9, H = 6;
    std::vector<Guide> g((size_t)W * H, hit_guide(3.0f, 1));
    for (float c : {0.5f, 0.25f, 0.75f, 2.0f, 0.0f}) {
      CHECK(rtwd::luminance((double)c, (double)c, (double)c) == (double)c, "luminance of grey %g", c);
      std::vector<Px> img((size_t)W * H, Px{c, c, c, kVarUnknown});
      const std::vector<float> v = estimate(img, guided ? &g : nullptr, W, H);
      for (size_t i = 0; i < v.size(); ++i) CHECK(bits(v[i]) == 0u, "grey %g, guided %d: var[%zu] = %g", c, guided, i, v[i]);
    }
    std::vector<Px> img((size_t)W * H, Px{0.3f, 0.7f, 0.2f, kVarUnknown});
    const double y = rtwd::luminance((double)0.3f, (double)0.7f, (double)0.2f);
    const std::vector<float> v = estimate(img, guided ? &g : nullptr, W, H);
    for (size_t i = 0; i < v.size(); ++i)
      CHECK(v[i] >= 0.0f && (double)v[i] <= std::ldexp(y * y, -46), "constant image, guided %d: var[%zu] = %g", guided, i, v[i]);
  }
  // 2. 1x1 and 2x1 stay unknown; 2x2 (four taps) gets a value.
  {
    std::vector<Px> a(1, Px{0.5f, 0.5f, 0.5f, kVarUnknown});
    CHECK(bits(estimate(a, nullptr, 1, 1)[0]) == bits(kVarUnknown), "1x1");
    std::vector<Px> b = {Px{0.1f, 0.1f, 0.1f, kVarUnknown}, Px{0.9f, 0.9f, 0.9f, kVarUnknown}};
    const std::vector<float> vb = estimate(b, nullptr, 2, 1);
    CHECK(bits(vb[0]) == bits(kVarUnknown) && bits(vb[1]) == bits(kVarUnknown), "2x1");
    const std::vector<float> vb2 = estimate(b, nullptr, 1, 2);
    CHECK(bits(vb2[0]) == bits(kVarUnknown) && bits(vb2[1]) == bits(kVarUnknown), "1x2");
    std::vector<Px> c = {Px{0.1f, 0.1f, 0.1f, kVarUnknown}, Px{0.9f, 0.9f, 0.9f, kVarUnknown},
                         Px{0.4f, 0.4f, 0.4f, kVarUnknown}, Px{0.6f, 0.6f, 0.6f, kVarUnknown}};
    const std::vector<float> vc = estimate(c, nullptr, 2, 2);
    for (int i = 0; i < 4; ++i) CHECK(vc[i] > 0.0f && bits(vc[i]) == bits(vc[0]), "2x2: var[%d] = %g", i, vc[i]);
  }
  // 3. 3x3 without guides: every pixel sees all nine taps with weight 1, so each
  //    is s2/9 - (s1/9)^2 in the stated order.
  {
    std::vector<Px> img(9);
    double sw = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < 9; ++i) {
      img[i] = Px{noise(3 * i), noise(3 * i + 1), noise(3 * i + 2), kVarUnknown};
      const double y = rtwd::luminance((double)img[i].r, (double)img[i].g, (double)img[i].b);
      sw += 1.0;
      s1 += 1.0 * y;
      s2 += 1.0 * (y * y);
    }
    const double m1 = s1 / sw;
    const float want = (float)fmax(0.0, s2 / sw - m1 * m1);
    const std::vector<float> v = estimate(img, nullptr, 3, 3);
    CHECK(want > 0.0f, "3x3: the hand-written value is %g", want);
    for (int i = 0; i < 9; ++i) CHECK(bits(v[i]) == bits(want), "3x3: var[%d] = %.9g, want %.9g", i, v[i], want);
  }
  // 4. Known pixels come back bit for bit (0, a denormal, a large value, -0
  //    counts as known: -0 >= 0); empty pixels stay empty, whatever their value
  //    below -1.5; and a huge rgb in an empty pixel changes no neighbour.
  {
    const int W = 11, H = 8;
    std::vector<Px> img((size_t)W * H);
    for (size_t i = 0; i < img.size(); ++i)
      img[i] = Px{noise(7 * i), noise(7 * i + 1), noise(7 * i + 2), kVarUnknown};
    const float known[] = {0.0f, 1e-42f, 3.25e7f, 0.0123f, -0.0f};
    for (int k = 0; k < 5; ++k) img[5 * k + 2].var = known[k];
    img[40].var = kVarEmpty, img[41].var = -7.5f;
    img[40].r = img[40].g = img[40].b = 0.0f;
    img[41].r = img[41].g = img[41].b = 0.0f;
    const std::vector<float> v = estimate(img, nullptr, W, H);
    for (int k = 0; k < 5; ++k) CHECK(bits(v[5 * k + 2]) == bits(known[k]), "known %g came back as %g", known[k], v[5 * k + 2]);
    CHECK(bits(v[40]) == bits(kVarEmpty) && bits(v[41]) == bits(-7.5f), "empty pixels: %g %g", v[40], v[41]);
    std::vector<Px> huge = img;
    huge[40].r = huge[40].g = huge[40].b = 1e30f;
    huge[41].r = std::nanf("");
    const std::vector<float> vh = estimate(huge, nullptr, W, H);
    for (size_t i = 0; i < v.size(); ++i) CHECK(bits(v[i]) == bits(vh[i]), "an empty pixel's rgb reached pixel %zu", i);
    int estimated = 0;
    for (size_t i = 0; i < v.size(); ++i) estimated += v[i] > 0.0f;
    CHECK(estimated == W * H - 4, "%d pixels estimated", estimated);  // (all but 0, -0 and the two empty)
  }
  // 5. Two constant regions (greys of exact sums, see 1) split along a hit /
  //    miss border: with guides 0 on both sides (the hard stop), without guides
  //    > 0 at the border and 0 away from it.
  {
    const int W = 16, H = 9;
    std::vector<Px> img((size_t)W * H);
    std::vector<Guide> g((size_t)W * H);
    Guide miss{};
    miss.albedo[0] = 0.7f, miss.albedo[1] = 0.8f, miss.albedo[2] = 1.0f;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const bool left = x < 8;
        img[(size_t)y * W + x] = left ? Px{0.25f, 0.25f, 0.25f, kVarUnknown} : Px{0.75f, 0.75f, 0.75f, kVarUnknown};
        g[(size_t)y * W + x] = left ? hit_guide(2.0f, 3) : miss;
      }
    const std::vector<float> vg = estimate(img, &g, W, H), vn = estimate(img, nullptr, W, H);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t i = (size_t)y * W + x;
        CHECK(bits(vg[i]) == 0u, "guided border: var(%d, %d) = %g", x, y, vg[i]);
        const bool near = x >= 5 && x <= 10;  // within 3 of the border between x = 7 and 8
        CHECK(near ? vn[i] > 0.0f : bits(vn[i]) == 0u, "unguided border: var(%d, %d) = %g", x, y, vn[i]);
      }
  }
  // 6. Scaling the image by 2 scales the estimate by exactly 4 (guided, with
  //    varying depths and normals so that the weights are not all 1).
  {
    const int W = 13, H = 10;
    std::vector<Px> img((size_t)W * H), img2((size_t)W * H);
    std::vector<Guide> g((size_t)W * H);
    for (int i = 0; i < W * H; ++i) {
      img[i] = Px{noise(5 * i), noise(5 * i + 1), noise(5 * i + 2), kVarUnknown};
      img2[i] = Px{2.0f * img[i].r, 2.0f * img[i].g, 2.0f * img[i].b, kVarUnknown};
      g[i] = hit_guide(2.0f + 0.3f * noise(5 * i + 3), 1);
      const float a = 0.2f * noise(5 * i + 4);
      g[i].n[0] = std::sin(a), g[i].n[2] = std::cos(a);
    }
    const std::vector<float> v = estimate(img, &g, W, H), v2 = estimate(img2, &g, W, H), vu = estimate(img, nullptr, W, H);
    int differ = 0;
    for (int i = 0; i < W * H; ++i) {
      CHECK(v[i] > 0.0f && bits(v2[i]) == bits(4.0f * v[i]), "scaling: var[%d] = %g, of the doubled image %g", i, v[i], v2[i]);
      differ += bits(v[i]) != bits(vu[i]);
    }
    CHECK(differ > W * H / 2, "the guides changed %d of %d estimates", differ, W * H);
  }
  // 7. A degenerate guide (a hit with a zero normal: tn = 0 for every tap, the
  //    centre included) keeps no tap: the pixel stays unknown, and is no NaN.
  {
    const int W = 5, H = 5;
    std::vector<Px> img((size_t)W * H, Px{0.5f, 0.5f, 0.5f, kVarUnknown});
    std::vector<Guide> g((size_t)W * H, hit_guide(1.0f, 1));
    g[12].n[2] = 0.0f;
    const std::vector<float> v = estimate(img, &g, W, H);
    CHECK(bits(v[12]) == bits(kVarUnknown), "degenerate centre: %g", v[12]);
    CHECK(bits(v[0]) == 0u, "its neighbours: %g", v[0]);
  }
  std::printf("denoise_spatial_check: bad %d/%d\n", g_bad, g_checks);
  return g_bad ? 1 : 0;
}
