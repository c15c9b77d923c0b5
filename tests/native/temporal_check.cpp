// temporal_check.cpp — temporal accumulation's arithmetic (csrc/rtw_temporal.hpp)
// with a plain C++ compiler, no HIP and no library.  tests/test_temporal_host.py
// builds and runs it, once more with the address and undefined-behaviour
// sanitizers.  It holds the header against the definition of rtw_hip.h stated a
// second time below (ref_pixel: straight-line code, its own projection), bit for
// bit on fuzzed frames, and checks the properties the header's users rely on:
// the first frame, a static camera's running mean, the projection's round trip,
// every rejection, and the half-pixel shift's weights.  The header's one addition
// to the definition (a tap of weight 0 does not count) is not in ref_pixel; what
// it is for has a check of its own (weightless_taps).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rtw_temporal.hpp"

using rtwt::Guide;
using rtwt::History;

static int g_bad = 0, g_checks = 0;
#define CHECK(cond, ...)                               \
  do {                                                 \
    ++g_checks;                                        \
    if (!(cond)) {                                     \
      ++g_bad;                                         \
      std::printf("FAIL %s:%d ", __FILE__, __LINE__);  \
      std::printf(__VA_ARGS__);                        \
      std::printf("\n");                               \
    }                                                  \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double rnd() {  // [0, 1)
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return (double)(g_rng >> 11) * 0x1p-53;
}
static double rnd(double a, double b) { return a + (b - a) * rnd(); }

struct Cam {
  double origin[3], h[3], v[3], llc[3];
};

// ---- the definition, a second time --------------------------------------------------
static bool ref_project(const Cam& c, const double pp[3], int W, int H, bool snap, double& fx, double& fy, double& tp) {
  const double qx = pp[0] - c.origin[0], qy = pp[1] - c.origin[1], qz = pp[2] - c.origin[2];
  if (!std::isfinite(qx) || !std::isfinite(qy) || !std::isfinite(qz)) return false;
  const double dx = c.llc[0] - c.origin[0], dy = c.llc[1] - c.origin[1], dz = c.llc[2] - c.origin[2];
  // n = h x v;  a = d0 x v;  b = h x d0
  const double nx = c.h[1] * c.v[2] - c.h[2] * c.v[1], ny = c.h[2] * c.v[0] - c.h[0] * c.v[2],
               nz = c.h[0] * c.v[1] - c.h[1] * c.v[0];
  const double ax = dy * c.v[2] - dz * c.v[1], ay = dz * c.v[0] - dx * c.v[2], az = dx * c.v[1] - dy * c.v[0];
  const double bx = c.h[1] * dz - c.h[2] * dy, by = c.h[2] * dx - c.h[0] * dz, bz = c.h[0] * dy - c.h[1] * dx;
  const double det = (qx * nx + qy * ny) + qz * nz;
  if (!std::isfinite(det) || det == 0.0) return false;
  const double mu = ((dx * nx + dy * ny) + dz * nz) / det;
  const double s = -((qx * ax + qy * ay) + qz * az) / det;
  const double t = -((qx * bx + qy * by) + qz * bz) / det;
  if (!std::isfinite(mu) || !std::isfinite(s) || !std::isfinite(t) || !(mu > 0.0)) return false;
  fx = s * (double)(W - 1) - 0.5;
  fy = ((double)(H - 1) + 0.5) - t * (double)(H - 1);
  if (snap) {
    const double rx = std::floor(fx + 0.5), ry = std::floor(fy + 0.5);
    if (std::fabs(fx - rx) <= 0x1p-10) fx = rx;
    if (std::fabs(fy - ry) <= 0x1p-10) fy = ry;
  }
  tp = 1.0 / mu;
  return true;
}

struct RefOut {
  History rec;
  float var;
  bool had_history;
};
static RefOut ref_pixel(int x, int y, int W, int H, double max_history, double depth_tol, double min_len_var,
                        const float* mean, const Guide& g, const History* hist, const double* pp, const Cam& prev,
                        bool same_cam) {
  const double c[3] = {mean[0], mean[1], mean[2]};
  const double Y = (0.2126 * c[0] + 0.7152 * c[1]) + 0.0722 * c[2];
  double fx = x, fy = y, tp = g.depth;
  bool valid = hist != nullptr;
  if (valid && g.prim != 0u && pp) valid = ref_project(prev, pp, W, H, true, fx, fy, tp);
  if (valid && g.prim == 0u) valid = same_cam;
  double ws = 0, sum[6] = {0, 0, 0, 0, 0, 0};
  if (valid && fx > -1.0 && fx < (double)W && fy > -1.0 && fy < (double)H) {
    const int x0 = (int)std::floor(fx), y0 = (int)std::floor(fy);
    const double wx = fx - std::floor(fx), wy = fy - std::floor(fy);
    const int tx[4] = {x0, x0 + 1, x0, x0 + 1}, ty[4] = {y0, y0, y0 + 1, y0 + 1};
    const double tw[4] = {(1.0 - wx) * (1.0 - wy), wx * (1.0 - wy), (1.0 - wx) * wy, wx * wy};
    for (int k = 0; k < 4; ++k) {  // (no rule about a weight of 0 here: see weightless_taps())
      if (tx[k] < 0 || tx[k] >= W || ty[k] < 0 || ty[k] >= H) continue;
      const History& r = hist[(size_t)ty[k] * W + tx[k]];
      if (!(r.len > 0.0f) || r.prim != g.prim) continue;
      if (g.prim != 0u && !(std::fabs((double)r.depth - tp) <= depth_tol * std::fmax((double)r.depth, tp))) continue;
      ws += tw[k];
      const double f[6] = {r.mean[0], r.mean[1], r.mean[2], r.len, r.m1, r.m2};
      for (int j = 0; j < 6; ++j) sum[j] += tw[k] * f[j];
    }
  }
  RefOut o;
  double len, m1, m2;
  o.had_history = !(ws < 0x1p-7);
  if (!o.had_history) {
    for (int j = 0; j < 3; ++j) o.rec.mean[j] = mean[j];
    len = 1.0, m1 = Y, m2 = Y * Y;
  } else {
    double hs[6];
    for (int j = 0; j < 6; ++j) hs[j] = sum[j] / ws;
    const double N = std::fmin(hs[3], max_history), a = 1.0 / (N + 1.0);
    for (int j = 0; j < 3; ++j) o.rec.mean[j] = (float)(hs[j] + a * (c[j] - hs[j]));
    len = N + 1.0;
    m1 = hs[4] + a * (Y - hs[4]);
    m2 = hs[5] + a * (Y * Y - hs[5]);
  }
  o.rec.len = (float)len, o.rec.m1 = (float)m1, o.rec.m2 = (float)m2;
  o.rec.depth = g.depth, o.rec.prim = g.prim;
  o.var = len >= min_len_var ? (float)(std::fmax(0.0, m2 - m1 * m1) / len) : -1.0f;
  return o;
}

// ---- the header over a frame (rtw_temporal_host's loop) ---------------------------
struct Frame {
  int W, H;
  std::vector<float> mean;
  std::vector<Guide> guides;
  std::vector<double> pp;  // empty: none
};
static void run(const Frame& f, const rtwt::Params& P, const std::vector<History>* hin, const Cam& prev, bool same_cam,
                std::vector<History>& hout, std::vector<float>& var) {
  const rtwt::Proj proj = rtwt::make_proj(prev.origin, prev.h, prev.v, prev.llc);
  hout.resize((size_t)f.W * f.H), var.resize((size_t)f.W * f.H);
  auto hist = [&](int x, int y) { return (*hin)[(size_t)y * f.W + x]; };
  for (int y = 0; y < f.H; ++y)
    for (int x = 0; x < f.W; ++x) {
      const size_t i = (size_t)y * f.W + x;
      const bool has_pp = !f.pp.empty();
      const rtwt::Out r = rtwt::accumulate_pixel(x, y, f.W, f.H, P, f.mean[3 * i], f.mean[3 * i + 1], f.mean[3 * i + 2],
                                                 f.guides[i], hin != nullptr, has_pp, has_pp ? f.pp[3 * i] : 0.0,
                                                 has_pp ? f.pp[3 * i + 1] : 0.0, has_pp ? f.pp[3 * i + 2] : 0.0, proj,
                                                 same_cam, hist);
      hout[i] = r.rec, var[i] = r.var;
    }
}

static Cam make_cam(const double o[3], const double u[3], const double v[3], const double w[3], double hw, double hh,
                    double focus) {
  Cam c;
  for (int k = 0; k < 3; ++k) {
    c.origin[k] = o[k], c.h[k] = u[k] * hw, c.v[k] = v[k] * hh;
    c.llc[k] = ((o[k] - c.h[k] / 2.0) - c.v[k] / 2.0) - w[k] * focus;
  }
  return c;
}
static Cam random_cam() {
  double w[3] = {rnd(-1, 1), rnd(-0.3, 0.3), rnd(-1, 1)}, up[3] = {0, 1, 0}, u[3], v[3];
  const double lw = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) + 1e-3;
  for (double& k : w) k /= lw;
  rtwt::cross3(up, w, u);
  const double lu = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) + 1e-3;
  for (double& k : u) k /= lu;
  rtwt::cross3(w, u, v);
  const double o[3] = {rnd(-5, 5), rnd(-5, 5), rnd(-5, 5)};
  return make_cam(o, u, v, w, rnd(0.5, 3), rnd(0.5, 3), rnd(1, 10));
}
static void pixel_point(const Cam& c, int W, int H, double px, double py, double depth, double out[3]) {
  const double s = (px + 0.5) / (double)(W - 1), t = (((double)(H - 1) - py) + 0.5) / (double)(H - 1);
  for (int k = 0; k < 3; ++k) out[k] = c.origin[k] + depth * (((c.llc[k] + c.h[k] * s) + c.v[k] * t) - c.origin[k]);
}
static Guide hit_guide(float depth, uint32_t prim) {
  Guide g{};
  g.n[2] = 1.0f, g.depth = depth, g.prim = prim;
  g.albedo[0] = g.albedo[1] = g.albedo[2] = 0.5f;
  return g;
}
static bool same_bytes(const History& a, float va, const History& b, float vb) {
  return std::memcmp(&a, &b, sizeof(History)) == 0 && std::memcmp(&va, &vb, 4) == 0;
}

static void fuzz() {
  long with_history = 0, without = 0;
  for (int trial = 0; trial < 150; ++trial) {
    Frame f;
    f.W = 2 + (int)(rnd() * 20), f.H = 2 + (int)(rnd() * 12);
    const size_t n = (size_t)f.W * f.H;
    const Cam cam = random_cam();
    Cam prev = (trial % 3 == 0) ? cam : random_cam();
    if (trial % 3 == 1) {  // a small camera move
      prev = cam;
      for (int k = 0; k < 3; ++k) prev.origin[k] += rnd(-0.05, 0.05), prev.llc[k] += rnd(-0.05, 0.05);
    }
    const bool same_cam = trial % 3 == 0;
    rtwt::Params P;
    const uint32_t mh = trial % 4 == 0 ? 0u : 1u + (uint32_t)(rnd() * 40);
    const double tol = trial % 2 ? 0.0 : rnd(0.01, 0.6);
    const uint32_t mlv = trial % 5 == 0 ? 0u : 2u + (uint32_t)(rnd() * 6);
    CHECK(rtwt::resolve(mh, tol, mlv, 0, P), "resolve");
    std::vector<History> hin(n);
    f.mean.resize(3 * n), f.guides.resize(n);
    if (trial % 4 != 3) f.pp.resize(3 * n);
    for (size_t i = 0; i < n; ++i) {
      const int x = (int)(i % f.W), y = (int)(i / f.W);
      for (int k = 0; k < 3; ++k) f.mean[3 * i + k] = (float)rnd(0, 2);
      const uint32_t prim = (uint32_t)(rnd() * 3);
      const double depth = rnd(1, 3);
      f.guides[i] = prim ? hit_guide((float)depth, prim) : Guide{};
      History& h = hin[i];
      for (float& m : h.mean) m = (float)rnd(0, 2);
      h.len = rnd() < 0.1 ? 0.0f : (float)(1 + (int)(rnd() * 50));
      h.m1 = (float)rnd(0, 2), h.m2 = h.m1 * h.m1 + (float)rnd(0, 0.5);
      h.prim = rnd() < 0.7 ? prim : (uint32_t)(rnd() * 3);
      h.depth = (float)(depth * rnd(0.9, 1.1));
      if (rnd() < 0.03) h.depth = NAN;
      if (!f.pp.empty()) {
        double p[3];
        pixel_point(cam, f.W, f.H, x + rnd(-1.5, 1.5), y + rnd(-1.5, 1.5), depth, p);
        const double r = rnd();
        if (r < 0.03) p[(int)(rnd() * 3)] = NAN;
        else if (r < 0.06) p[(int)(rnd() * 3)] = INFINITY;
        else if (r < 0.09) for (int k = 0; k < 3; ++k) p[k] = prev.origin[k];
        else if (r < 0.12) for (int k = 0; k < 3; ++k) p[k] = 2.0 * prev.origin[k] - p[k];
        for (int k = 0; k < 3; ++k) f.pp[3 * i + k] = p[k];
      }
    }
    for (int first = 0; first < 2; ++first) {
      std::vector<History> hout;
      std::vector<float> var;
      run(f, P, first ? nullptr : &hin, prev, same_cam, hout, var);
      for (size_t i = 0; i < n; ++i) {
        const RefOut r = ref_pixel((int)(i % f.W), (int)(i / f.W), f.W, f.H, P.max_history, P.depth_tol, P.min_len_var,
                                   &f.mean[3 * i], f.guides[i], first ? nullptr : hin.data(),
                                   f.pp.empty() ? nullptr : &f.pp[3 * i], prev, same_cam);
        CHECK(same_bytes(hout[i], var[i], r.rec, r.var), "fuzz trial %d pixel %zu: header and definition differ", trial, i);
        if (!first) (r.had_history ? with_history : without)++;
        if (first) {
          CHECK(std::memcmp(hout[i].mean, &f.mean[3 * i], 12) == 0 && hout[i].len == 1.0f && var[i] == -1.0f,
                "first frame: pixel %zu", i);
        }
      }
    }
  }
  std::printf("fuzz: %ld pixels with history, %ld without\n", with_history, without);
  CHECK(with_history > 1000 && without > 1000, "the fuzz reaches both branches");
}

static void static_camera() {
  const int W = 7, H = 5, K = 8;
  const size_t n = (size_t)W * H;
  const Cam cam = random_cam();
  for (uint32_t mh : {0u, 3u}) {
    rtwt::Params P;
    CHECK(rtwt::resolve(mh, 0, 0, 0, P), "resolve");
    Frame f;
    f.W = W, f.H = H, f.mean.resize(3 * n), f.guides.resize(n);
    for (size_t i = 0; i < n; ++i) f.guides[i] = i % 4 ? hit_guide((float)rnd(1, 3), 1u + (uint32_t)(i % 3)) : Guide{};
    std::vector<History> h[2];
    std::vector<float> var;
    std::vector<double> rm(3 * n, 0.0);
    for (int k = 0; k < K; ++k) {
      for (size_t j = 0; j < 3 * n; ++j) {
        f.mean[j] = (float)rnd(0, 2);
        rm[j] += ((double)f.mean[j] - rm[j]) / (double)(k + 1);
      }
      run(f, P, k ? &h[(k + 1) & 1] : nullptr, cam, true, h[k & 1], var);
      for (size_t i = 0; i < n; ++i) {
        const History& r = h[k & 1][i];
        if (mh == 0u) {
          CHECK(r.len == (float)(k + 1), "static: len %g at frame %d", r.len, k);
          for (int c = 0; c < 3; ++c)
            CHECK(std::fabs((double)r.mean[c] - rm[3 * i + c]) <= 1e-6 * std::fabs(rm[3 * i + c]),
                  "static: mean %.9g against the running mean %.9g (frame %d)", r.mean[c], rm[3 * i + c], k);
          CHECK((var[i] >= 0.0f) == (k + 1 >= 4), "static: variance %g known from min_len_var on (frame %d)", var[i], k);
        } else {
          CHECK(r.len == (float)std::min(k + 1, 4), "max_history 3: len %g at frame %d", r.len, k);
        }
      }
    }
  }
}

static void round_trip() {
  for (int trial = 0; trial < 200; ++trial) {
    const Cam cam = random_cam();
    const int W = 2 + (int)(rnd() * 1300), H = 2 + (int)(rnd() * 700);
    const int x = (int)(rnd() * W), y = (int)(rnd() * H);
    const double depth = rnd(0.01, 100);
    double p[3], fx, fy, tp;
    pixel_point(cam, W, H, x, y, depth, p);
    CHECK(ref_project(cam, p, W, H, false, fx, fy, tp), "round trip: invalid");
    CHECK(std::fabs(fx - x) <= 1e-6 && std::fabs(fy - y) <= 1e-6, "round trip: (%d, %d) lands at (%.12g, %.12g)", x, y, fx, fy);
    const rtwt::Proj proj = rtwt::make_proj(cam.origin, cam.h, cam.v, cam.llc);
    CHECK(rtwt::project(proj, p[0], p[1], p[2], W, H, fx, fy, tp), "round trip: invalid");
    CHECK(fx == (double)x && fy == (double)y, "round trip: the snap leaves (%.17g, %.17g) for (%d, %d)", fx, fy, x, y);
    CHECK(std::fabs(tp - depth) <= 1e-9 * depth, "round trip: tp %.17g for depth %.17g", tp, depth);
  }
}

// An axis-aligned camera whose numbers are exact: s = (fx + 0.5) / 4 for W = 5.
static Cam exact_cam() {
  Cam c;
  const double o[3] = {0, 0, 0}, h[3] = {4, 0, 0}, v[3] = {0, 4, 0}, l[3] = {-2, -2, -1};
  for (int k = 0; k < 3; ++k) c.origin[k] = o[k], c.h[k] = h[k], c.v[k] = v[k], c.llc[k] = l[k];
  return c;
}

static void rejections_and_shift() {
  const int W = 5, H = 5;
  const size_t n = (size_t)W * H;
  const Cam cam = exact_cam();
  rtwt::Params P;
  CHECK(rtwt::resolve(0, 0, 0, 0, P), "resolve");
  Frame f;
  f.W = W, f.H = H, f.mean.resize(3 * n), f.guides.assign(n, hit_guide(2.0f, 1u)), f.pp.resize(3 * n);
  for (size_t j = 0; j < 3 * n; ++j) f.mean[j] = (float)rnd(0, 2);
  auto fill_pp = [&](double dx, double dy) {
    for (size_t i = 0; i < n; ++i) pixel_point(cam, W, H, (double)(i % W) + dx, (double)(i / W) + dy, 2.0, &f.pp[3 * i]);
  };
  std::vector<History> hin(n);
  for (size_t i = 0; i < n; ++i) {
    History& h = hin[i];
    for (float& m : h.mean) m = (float)rnd(0, 2);
    h.len = 3.0f, h.m1 = (float)rnd(0, 1), h.m2 = (float)rnd(1, 2), h.depth = 2.0f, h.prim = 1u;
  }
  std::vector<History> none, got;
  std::vector<float> none_var, got_var;
  fill_pp(0, 0);
  run(f, P, nullptr, cam, true, none, none_var);
  const size_t c = 2 * W + 2;  // the centre pixel
  auto expect_none = [&](const char* what) {
    run(f, P, &hin, cam, true, got, got_var);
    CHECK(same_bytes(got[c], got_var[c], none[c], none_var[c]), "rejection: %s keeps history (len %g)", what, got[c].len);
  };
  run(f, P, &hin, cam, true, got, got_var);
  CHECK(got[c].len == 4.0f, "the accepted case: len %g", got[c].len);
  {
    const std::vector<History> keep = hin;
    for (History& h : hin) h.prim = 2u;
    expect_none("a tap of another prim");
    hin = keep;
    for (History& h : hin) h.depth = (float)(2.0 * (1.0 + 2.0 * P.depth_tol));
    expect_none("a depth off by twice depth_tol");
    hin = keep;
    for (History& h : hin) h.len = 0.0f;
    expect_none("records without history");
    hin = keep;
  }
  const std::vector<double> keep_pp = f.pp;
  for (int k = 0; k < 3; ++k) f.pp[3 * c + k] = -keep_pp[3 * c + k];  // (origin 0: the mirrored point)
  expect_none("a point behind the previous camera");
  f.pp[3 * c] = 1.0, f.pp[3 * c + 1] = 0.0, f.pp[3 * c + 2] = 0.0;  // q = (1, 0, 0), n = (0, 0, 16): det 0
  expect_none("determinant 0 (q in the image plane's direction)");
  f.pp[3 * c] = 0.0;  // q = 0
  expect_none("determinant 0 (the camera's origin)");
  f.pp = keep_pp, f.pp[3 * c + 1] = NAN;
  expect_none("a NaN point");
  f.pp = keep_pp;
  pixel_point(cam, W, H, 40.0, -30.0, 2.0, &f.pp[3 * c]);
  expect_none("all four taps outside the image");
  f.pp = keep_pp;
  // half a pixel: weights 1/4 each
  fill_pp(0.5, 0.5);
  run(f, P, &hin, cam, true, got, got_var);
  const History* t[4] = {&hin[2 * W + 2], &hin[2 * W + 3], &hin[3 * W + 2], &hin[3 * W + 3]};
  CHECK(got[c].len == 4.0f, "half-pixel shift: len %g", got[c].len);
  for (int k = 0; k < 3; ++k) {
    const double avg = ((double)t[0]->mean[k] + (double)t[1]->mean[k] + (double)t[2]->mean[k] + (double)t[3]->mean[k]) / 4.0;
    const float want = (float)(avg + 0.25 * ((double)f.mean[3 * c + k] - avg));
    CHECK(got[c].mean[k] == want, "half-pixel shift: channel %d is %.9g, the exact average gives %.9g", k, got[c].mean[k], want);
  }
  rtwt::Params Q;
  CHECK(!rtwt::resolve(4097, 0, 0, 0, Q) && !rtwt::resolve(0, -1.0, 0, 0, Q) && !rtwt::resolve(0, NAN, 0, 0, Q) &&
            !rtwt::resolve(0, 0, 1, 0, Q) && !rtwt::resolve(0, 0, 0, 1, Q) && rtwt::resolve(4096, 1.0, 2, 0, Q),
        "option ranges");
}

// The one rule the header adds to the definition: a tap also needs a weight > 0 to count.  ref_pixel does not
// have it, and on finite records it cannot matter (0 * r adds nothing to a sum, which the fuzz holds bit for bit
// on its snapped positions).  What it is for is checked here on its own: at a snapped position the three taps of
// weight 0 may hold anything — NaN, infinity — and the pixel still gets the bytes it gets beside clean records,
// where the definition's 0 * NaN would make the whole sum NaN.
static void weightless_taps() {
  const int W = 5, H = 5;
  const size_t n = (size_t)W * H, c = 2 * W + 2;
  const Cam cam = exact_cam();
  rtwt::Params P;
  CHECK(rtwt::resolve(0, 0, 0, 0, P), "resolve");
  Frame f;
  f.W = W, f.H = H, f.mean.resize(3 * n), f.guides.assign(n, hit_guide(2.0f, 1u));
  for (size_t j = 0; j < 3 * n; ++j) f.mean[j] = (float)rnd(0, 2);
  std::vector<History> hin(n);
  for (History& h : hin) {
    for (float& m : h.mean) m = (float)rnd(0, 2);
    h.len = 3.0f, h.m1 = (float)rnd(0, 1), h.m2 = (float)rnd(1, 2), h.depth = 2.0f, h.prim = 1u;
  }
  std::vector<History> clean, got;
  std::vector<float> clean_var, got_var;
  for (int with_pp = 0; with_pp < 2; ++with_pp) {  // no point buffer, and points that snap onto their own pixel
    f.pp.clear();
    if (with_pp) {
      f.pp.resize(3 * n);
      for (size_t i = 0; i < n; ++i) pixel_point(cam, W, H, (double)(i % W) + 0x1p-12, (double)(i / W) - 0x1p-12, 2.0, &f.pp[3 * i]);
    }
    std::vector<History> dirty = hin;
    for (size_t i : {c - W - 1, c - W, c - W + 1, c - 1, c + 1, c + W - 1, c + W, c + W + 1}) {  // every neighbour of c
      dirty[i].mean[0] = NAN, dirty[i].mean[1] = INFINITY, dirty[i].m1 = NAN, dirty[i].m2 = -INFINITY;
    }
    run(f, P, &hin, cam, true, clean, clean_var);
    run(f, P, &dirty, cam, true, got, got_var);
    CHECK(clean[c].len == 4.0f, "weightless taps: the clean case has len %g", clean[c].len);
    CHECK(same_bytes(got[c], got_var[c], clean[c], clean_var[c]), "weightless taps: a record of weight 0 leaked (with_pp %d)", with_pp);
    const RefOut r = ref_pixel(2, 2, W, H, P.max_history, P.depth_tol, P.min_len_var, &f.mean[3 * c], f.guides[c], hin.data(),
                               with_pp ? &f.pp[3 * c] : nullptr, cam, true);
    CHECK(same_bytes(clean[c], clean_var[c], r.rec, r.var), "weightless taps: the clean case against the definition");
  }
}

int main() {
  fuzz();
  weightless_taps();
  static_camera();
  round_trip();
  rejections_and_shift();
  std::printf("temporal_check: bad %d/%d\n", g_bad, g_checks);
  return g_bad ? 1 : 0;
}
