// temporal_clamp_check.cpp — the clamped temporal accumulation's arithmetic
// (csrc/rtw_temporal_clamp.hpp) with a plain C++ compiler, no HIP and no library.
// tests/test_temporal_clamp_host.py builds and runs it, once more with the address
// and undefined-behaviour sanitizers.  It holds the header against the definition
// of rtw_hip.h stated a second time below (ref_pixel: straight-line code, its own
// projection and its own window loop with an explicit in-image test), bit for bit
// on fuzzed frames, and checks what the header's users rely on: a clamp that does
// not bite is the unclamped path, a step change is followed at once, every output
// stays inside the window's range or towards the current value, the image's
// border and a bad pixel are one rule, noise still averages out on a still image
// while a changed image is caught up with, and the option ranges.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rtw_temporal_clamp.hpp"

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

static uint64_t g_rng = 0xD1B54A32D192ED03ull;
static double rnd() {  // [0, 1)
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return (double)(g_rng >> 11) * 0x1p-53;
}
static double rnd(double a, double b) { return a + (b - a) * rnd(); }
static double gauss() {  // Box-Muller
  const double u = 1.0 - rnd(), v = rnd();
  return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v);
}

struct Cam {
  double origin[3], h[3], v[3], llc[3];
};

// ---- the definition, a second time --------------------------------------------------
static bool ref_project(const Cam& c, const double pp[3], int W, int H, double& fx, double& fy, double& tp) {
  const double qx = pp[0] - c.origin[0], qy = pp[1] - c.origin[1], qz = pp[2] - c.origin[2];
  if (!std::isfinite(qx) || !std::isfinite(qy) || !std::isfinite(qz)) return false;
  const double dx = c.llc[0] - c.origin[0], dy = c.llc[1] - c.origin[1], dz = c.llc[2] - c.origin[2];
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
  const double rx = std::floor(fx + 0.5), ry = std::floor(fy + 0.5);
  if (std::fabs(fx - rx) <= 0x1p-10) fx = rx;
  if (std::fabs(fy - ry) <= 0x1p-10) fy = ry;
  tp = 1.0 / mu;
  return true;
}

static float to_f32(double v) {  // any NaN is stored as the one quiet NaN
  const uint32_t q = 0x7FC00000u;
  float f = (float)v;
  if (std::isnan(v)) std::memcpy(&f, &q, 4);
  return f;
}
static double lum(const double c[3]) { return (0.2126 * c[0] + 0.7152 * c[1]) + 0.0722 * c[2]; }

struct RefOut {
  History rec;
  float var;
  bool had_history, changed;
  int n;             // counted window pixels
  double lo[3], hi[3];
};
// gamma < 0: no clamp step at all (rtw_temporal.hpp's definition).
static RefOut ref_pixel(int x, int y, int W, int H, double max_history, double depth_tol, double min_len_var, double gamma,
                        int radius, const float* image, const Guide& g, const History* hist, const double* pp,
                        const Cam& prev, bool same_cam) {
  const float* mean = image + 3 * ((size_t)y * W + x);
  const double c[3] = {mean[0], mean[1], mean[2]};
  const double Y = lum(c);
  double fx = x, fy = y, tp = g.depth;
  bool valid = hist != nullptr;
  if (valid && g.prim != 0u && pp) valid = ref_project(prev, pp, W, H, fx, fy, tp);
  if (valid && g.prim == 0u) valid = same_cam;
  double ws = 0, sum[6] = {0, 0, 0, 0, 0, 0};
  if (valid && fx > -1.0 && fx < (double)W && fy > -1.0 && fy < (double)H) {
    const int x0 = (int)std::floor(fx), y0 = (int)std::floor(fy);
    const double wx = fx - std::floor(fx), wy = fy - std::floor(fy);
    const int tx[4] = {x0, x0 + 1, x0, x0 + 1}, ty[4] = {y0, y0, y0 + 1, y0 + 1};
    const double tw[4] = {(1.0 - wx) * (1.0 - wy), wx * (1.0 - wy), (1.0 - wx) * wy, wx * wy};
    for (int k = 0; k < 4; ++k) {
      if (!(tw[k] > 0.0) || tx[k] < 0 || tx[k] >= W || ty[k] < 0 || ty[k] >= H) continue;
      const History& r = hist[(size_t)ty[k] * W + tx[k]];
      if (!(r.len > 0.0f) || r.prim != g.prim) continue;
      if (g.prim != 0u && !(std::fabs((double)r.depth - tp) <= depth_tol * std::fmax((double)r.depth, tp))) continue;
      ws += tw[k];
      const double f[6] = {r.mean[0], r.mean[1], r.mean[2], r.len, r.m1, r.m2};
      for (int j = 0; j < 6; ++j) sum[j] += tw[k] * f[j];
    }
  }
  RefOut o{};
  double len, m1, m2;
  o.had_history = !(ws < 0x1p-7);
  if (!o.had_history) {
    for (int j = 0; j < 3; ++j) o.rec.mean[j] = mean[j];
    len = 1.0, m1 = Y, m2 = Y * Y;
  } else {
    double hs[6];
    for (int j = 0; j < 6; ++j) hs[j] = sum[j] / ws;
    if (gamma >= 0.0) {
      double s[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
      for (int qy = y - radius; qy <= y + radius; ++qy)
        for (int qx = x - radius; qx <= x + radius; ++qx) {
          if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;  // outside the image
          const float* q = image + 3 * ((size_t)qy * W + qx);
          if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2])) continue;
          ++o.n;
          for (int j = 0; j < 3; ++j) s[j] += (double)q[j], s2[j] += (double)q[j] * (double)q[j];
        }
      if (o.n >= 4) {
        double hc[3];
        for (int j = 0; j < 3; ++j) {
          const double mu = s[j] / (double)o.n;
          const double sg = std::sqrt(std::fmax(0.0, s2[j] / (double)o.n - mu * mu));
          o.lo[j] = mu - gamma * sg, o.hi[j] = mu + gamma * sg;
          hc[j] = std::fmin(std::fmax(hs[j], o.lo[j]), o.hi[j]);
          if (hc[j] != hs[j]) o.changed = true;
        }
        if (o.changed) {
          const double d = lum(hc) - lum(hs);
          hs[5] = (hs[5] + (2.0 * hs[4]) * d) + d * d;
          hs[4] = hs[4] + d;
          for (int j = 0; j < 3; ++j) hs[j] = hc[j];
        }
      }
    }
    const double N = std::fmin(hs[3], max_history), a = 1.0 / (N + 1.0);
    for (int j = 0; j < 3; ++j) o.rec.mean[j] = to_f32(hs[j] + a * (c[j] - hs[j]));
    len = N + 1.0;
    m1 = hs[4] + a * (Y - hs[4]);
    m2 = hs[5] + a * (Y * Y - hs[5]);
  }
  o.rec.len = (float)len, o.rec.m1 = to_f32(m1), o.rec.m2 = to_f32(m2);
  o.rec.depth = g.depth, o.rec.prim = g.prim;
  o.var = len >= min_len_var ? (float)(std::fmax(0.0, m2 - m1 * m1) / len) : -1.0f;
  return o;
}

// ---- the headers over a frame (the host entries' loops) -----------------------------
struct Frame {
  int W, H;
  std::vector<float> mean;
  std::vector<Guide> guides;
  std::vector<double> pp;  // empty: none
};
// K == nullptr: rtw_temporal.hpp's accumulate_pixel (the unclamped call).
static void run(const Frame& f, const rtwt::Params& P, const rtwt::Clamp* K, const std::vector<History>* hin,
                const Cam& prev, bool same_cam, std::vector<History>& hout, std::vector<float>& var) {
  const rtwt::Proj proj = rtwt::make_proj(prev.origin, prev.h, prev.v, prev.llc);
  hout.resize((size_t)f.W * f.H), var.resize((size_t)f.W * f.H);
  auto hist = [&](int x, int y) { return (*hin)[(size_t)y * f.W + x]; };
  auto cur = [&](int x, int y) {
    if (x < 0 || x >= f.W || y < 0 || y >= f.H) return rtwt::Rgb{NAN, NAN, NAN};
    const float* p = &f.mean[3 * ((size_t)y * f.W + x)];
    return rtwt::Rgb{p[0], p[1], p[2]};
  };
  for (int y = 0; y < f.H; ++y)
    for (int x = 0; x < f.W; ++x) {
      const size_t i = (size_t)y * f.W + x;
      const bool has_pp = !f.pp.empty();
      const double p0 = has_pp ? f.pp[3 * i] : 0.0, p1 = has_pp ? f.pp[3 * i + 1] : 0.0, p2 = has_pp ? f.pp[3 * i + 2] : 0.0;
      const rtwt::Out r =
          K ? rtwt::accumulate_pixel_clamped(x, y, f.W, f.H, P, K->gamma, K->radius, f.guides[i], hin != nullptr, has_pp,
                                             p0, p1, p2, proj, same_cam, hist, cur)
            : rtwt::accumulate_pixel(x, y, f.W, f.H, P, f.mean[3 * i], f.mean[3 * i + 1], f.mean[3 * i + 2], f.guides[i],
                                     hin != nullptr, has_pp, p0, p1, p2, proj, same_cam, hist);
      hout[i] = r.rec, var[i] = r.var;
    }
}

static Cam look_cam(double ox, double oy, double oz, double aspect) {  // towards the origin, 20 degrees
  const double o[3] = {ox, oy, oz};
  double w[3] = {ox, oy, oz}, up[3] = {0, 1, 0}, u[3], v[3];
  const double lw = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  for (double& k : w) k /= lw;
  rtwt::cross3(up, w, u);
  const double lu = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for (double& k : u) k /= lu;
  rtwt::cross3(w, u, v);
  const double hh = 2.0 * std::tan(10.0 * 3.141592653589793 / 180.0) * 10.0, hw = aspect * hh;
  Cam c;
  for (int k = 0; k < 3; ++k) {
    c.origin[k] = o[k], c.h[k] = u[k] * hw, c.v[k] = v[k] * hh;
    c.llc[k] = ((o[k] - c.h[k] / 2.0) - c.v[k] / 2.0) - w[k] * 10.0;
  }
  return c;
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

// The fuzz of tests/test_gpu_temporal.py make_case: guides in blocks of four primitives and a block of misses,
// a depth step inside the blocks, previous points a pixel or so away with NaN points, the camera's origin,
// points behind it, points far outside and points off in depth among them; the history is a first frame's.
struct Case {
  Frame f;
  Cam cam, cam_moved;
  std::vector<History> hin;
};
static Case make_case(int W, int H, bool bad_pixels) {
  Case c;
  Frame& f = c.f;
  f.W = W, f.H = H;
  const size_t n = (size_t)W * H;
  c.cam = look_cam(13, 2, 3, (double)W / H), c.cam_moved = look_cam(13.02, 2.01, 3, (double)W / H);
  f.mean.resize(3 * n), f.guides.resize(n), f.pp.resize(3 * n), c.hin.resize(n);
  for (size_t i = 0; i < n; ++i) {
    const int x = (int)(i % W), y = (int)(i / W);
    const uint32_t prim = 1u + (x >= W / 2) + 2u * (y >= (2 * H) / 3);
    const float depth = (float)(2.0 + 0.004 * x + 0.003 * y + 1.5 * (x >= (3 * W) / 4));
    const bool miss = x < std::max(1, W / 5) && y < std::max(1, H / 2);
    f.guides[i] = miss ? Guide{} : hit_guide(depth, prim);
    for (int k = 0; k < 3; ++k) f.mean[3 * i + k] = (float)rnd(0, 2);
    History& h = c.hin[i];  // a first frame of other means
    for (float& m : h.mean) m = (float)rnd(0, 2);
    const double hm[3] = {h.mean[0], h.mean[1], h.mean[2]};
    h.len = 1.0f + (float)(int)(rnd() * 6), h.m1 = (float)lum(hm), h.m2 = (float)(lum(hm) * lum(hm) + rnd(0, 0.2));
    h.depth = f.guides[i].depth, h.prim = f.guides[i].prim;
    double d = depth, p[3];
    const double kind = rnd();
    if (kind >= 0.16 && kind < 0.22) d *= 1.04;
    if (kind >= 0.22 && kind < 0.28) d *= 0.96;
    pixel_point(c.cam, W, H, x + rnd(-1.2, 1.2), y + rnd(-1.2, 1.2), d, p);
    if (kind < 0.04) p[0] = p[1] = p[2] = NAN;
    else if (kind < 0.08) for (int k = 0; k < 3; ++k) p[k] = c.cam.origin[k];
    else if (kind < 0.12) for (int k = 0; k < 3; ++k) p[k] = 2.0 * c.cam.origin[k] - p[k];
    else if (kind < 0.16) pixel_point(c.cam, W, H, x + 5.0 * W, y - 4.0 * H, 3.0, p);
    for (int k = 0; k < 3; ++k) f.pp[3 * i + k] = p[k];
  }
  if (bad_pixels) {  // a few non-finite pixels in the current mean
    const int k = std::max(1, (int)n / 16);
    for (int j = 0; j < k; ++j) f.mean[3 * (size_t)(rnd() * n) + (int)(rnd() * 3)] = j % 3 == 0 ? INFINITY : j % 3 == 1 ? -INFINITY : NAN;
  }
  return c;
}

static const int kSizes[4][2] = {{2, 2}, {5, 3}, {67, 9}, {130, 5}};
static const double kGammas[3] = {0.5, 1.0, 3.0};

static void second_statement_and_containment() {
  long with_history = 0, without = 0, clamped = 0, small_n = 0, contained = 0;
  for (const auto& wh : kSizes)
    for (int bad = 0; bad < 2; ++bad) {
      const Case c = make_case(wh[0], wh[1], bad != 0);
      const Frame& f = c.f;
      const size_t n = (size_t)f.W * f.H;
      for (int mode = 0; mode < 3; ++mode) {  // fuzzed points, fuzzed points under a moved camera, nothing moved
        Frame fm = f;
        if (mode == 2) fm.pp.clear();
        const Cam& prev = mode == 1 ? c.cam_moved : c.cam;
        const bool same_cam = mode != 1;
        rtwt::Params P;
        CHECK(rtwt::resolve(0, 0, 2, 0, P), "resolve");
        for (int r = 1; r <= 3; ++r)
          for (double gamma : kGammas) {
            rtwt::Clamp K;
            CHECK(rtwt::resolve_clamp(gamma, (uint32_t)r, 0, K) && K.gamma == gamma && K.radius == r, "resolve_clamp");
            std::vector<History> hout;
            std::vector<float> var;
            run(fm, P, &K, &c.hin, prev, same_cam, hout, var);
            for (size_t i = 0; i < n; ++i) {
              const int x = (int)(i % f.W), y = (int)(i / f.W);
              const RefOut o = ref_pixel(x, y, f.W, f.H, P.max_history, P.depth_tol, P.min_len_var, gamma, r, fm.mean.data(),
                                         fm.guides[i], c.hin.data(), fm.pp.empty() ? nullptr : &fm.pp[3 * i], prev, same_cam);
              CHECK(same_bytes(hout[i], var[i], o.rec, o.var), "%dx%d bad %d mode %d r %d gamma %g pixel %zu: header and definition differ",
                    f.W, f.H, bad, mode, r, gamma, i);
              (o.had_history ? with_history : without)++;
              if (!o.had_history) continue;
              if (o.n < 4) {
                ++small_n;
                continue;
              }
              clamped += o.changed;
              const float* cm = &fm.mean[3 * i];
              if (!std::isfinite(cm[0]) || !std::isfinite(cm[1]) || !std::isfinite(cm[2])) continue;
              ++contained;
              for (int j = 0; j < 3; ++j) {  // between the clamped history and the current value, one f32 ulp wider
                const float lo = std::nextafterf((float)std::fmin(o.lo[j], (double)cm[j]), -INFINITY);
                const float hi = std::nextafterf((float)std::fmax(o.hi[j], (double)cm[j]), INFINITY);
                CHECK(hout[i].mean[j] >= lo && hout[i].mean[j] <= hi, "containment: %dx%d r %d gamma %g pixel %zu channel %d: %.9g outside [%.9g, %.9g]",
                      f.W, f.H, r, gamma, i, j, hout[i].mean[j], lo, hi);
              }
            }
          }
      }
    }
  std::printf("fuzz: %ld pixels with history (%ld clamped, %ld with n < 4, %ld held to their range), %ld without\n", with_history,
              clamped, small_n, contained, without);
  CHECK(with_history > 10000 && without > 10000 && clamped > 5000 && contained > 10000, "the fuzz reaches every branch");
}

// gamma = 9e29 on finite frames: no channel changes, no moment moves, the bytes are accumulate_pixel's.
static void identity() {
  for (const auto& wh : kSizes) {
    const Case c = make_case(wh[0], wh[1], false);
    rtwt::Params P;
    CHECK(rtwt::resolve(0, 0, 2, 0, P), "resolve");
    for (int r = 1; r <= 3; ++r) {
      rtwt::Clamp K;
      CHECK(rtwt::resolve_clamp(9e29, (uint32_t)r, 0, K), "resolve_clamp 9e29");
      std::vector<History> a, b;
      std::vector<float> va, vb;
      run(c.f, P, &K, &c.hin, c.cam, true, a, va);
      run(c.f, P, nullptr, &c.hin, c.cam, true, b, vb);
      bool same = true;
      for (size_t i = 0; i < a.size(); ++i) same = same && same_bytes(a[i], va[i], b[i], vb[i]);
      CHECK(same, "identity: gamma 9e29 at %dx%d r %d differs from the unclamped call", wh[0], wh[1], r);
      run(c.f, P, &K, nullptr, c.cam, true, a, va);  // the first frame
      run(c.f, P, nullptr, nullptr, c.cam, true, b, vb);
      same = true;
      for (size_t i = 0; i < a.size(); ++i) same = same && same_bytes(a[i], va[i], b[i], vb[i]);
      CHECK(same, "identity: the first frame at %dx%d r %d", wh[0], wh[1], r);
    }
  }
}

static Frame constant_frame(int W, int H, const float v[3]) {
  Frame f;
  f.W = W, f.H = H;
  const size_t n = (size_t)W * H;
  f.mean.resize(3 * n), f.guides.assign(n, hit_guide(2.0f, 1u));
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) f.mean[3 * i + k] = v[k];
  return f;
}
static std::vector<History> constant_history(size_t n, const float v[3], float len) {
  const double d[3] = {v[0], v[1], v[2]};
  History h{};
  for (int k = 0; k < 3; ++k) h.mean[k] = v[k];
  h.len = len, h.m1 = (float)lum(d), h.m2 = (float)(lum(d) * lum(d)), h.depth = 2.0f, h.prim = 1u;
  return std::vector<History>(n, h);
}

// A history of a constant image A, the frame a constant image B: the window's sigma is 0, the history becomes B.
static void step_change() {
  const int W = 7, H = 5;
  const size_t n = (size_t)W * H;
  const float A[3] = {0.8f, 0.3f, 1.7f}, B[3] = {0.1f, 1.3f, 0.45f};
  const Frame f = constant_frame(W, H, B);
  const std::vector<History> hin = constant_history(n, A, 8.0f);
  const Cam cam = look_cam(13, 2, 3, (double)W / H);
  rtwt::Params P;
  CHECK(rtwt::resolve(0, 0, 0, 0, P), "resolve");
  const double Bd[3] = {B[0], B[1], B[2]}, YB = lum(Bd);
  for (double gamma : {0.25, 1.0, 3.0, 1000.0})
    for (int r = 1; r <= 3; ++r) {
      const rtwt::Clamp K{gamma, r};
      std::vector<History> got;
      std::vector<float> var;
      run(f, P, &K, &hin, cam, true, got, var);
      for (size_t i = 0; i < n; ++i) {
        CHECK(std::memcmp(got[i].mean, B, 12) == 0, "step change: gamma %g r %d pixel %zu is %.9g %.9g %.9g", gamma, r, i,
              got[i].mean[0], got[i].mean[1], got[i].mean[2]);
        CHECK(std::fabs((double)got[i].m1 - YB) <= 1e-6 * YB && got[i].len == 9.0f, "step change: m1 %.9g for %.9g, len %g", got[i].m1, YB, got[i].len);
        CHECK(var[i] >= 0.0f && var[i] <= 1e-6f, "step change: the variance of constant images is %.9g", var[i]);
      }
    }
  std::vector<History> got;
  std::vector<float> var;
  run(f, P, nullptr, &hin, cam, true, got, var);
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k)
      CHECK(got[i].mean[k] == (float)((double)A[k] + (1.0 / 9.0) * ((double)B[k] - (double)A[k])), "step change: the unclamped call lags at A + (B - A) / 9");
}

static void borders_and_skips() {
  const Cam cam = look_cam(13, 2, 3, 1.0);
  rtwt::Params P;
  CHECK(rtwt::resolve(0, 0, 0, 0, P), "resolve");
  const rtwt::Clamp K{1.0, 1};
  std::vector<History> got, plain;
  std::vector<float> var, plain_var;
  {  // 2x2, r = 1: every window holds the four pixels, and every pixel is clamped
    const float far[3] = {10.0f, 10.0f, 10.0f};
    Frame f = constant_frame(2, 2, far);
    for (float& m : f.mean) m = (float)rnd(0, 1);
    const std::vector<History> hin = constant_history(4, far, 8.0f);
    run(f, P, &K, &hin, cam, true, got, var);
    run(f, P, nullptr, &hin, cam, true, plain, plain_var);
    for (size_t i = 0; i < 4; ++i) {
      const RefOut o = ref_pixel((int)(i % 2), (int)(i / 2), 2, 2, P.max_history, P.depth_tol, P.min_len_var, 1.0, 1, f.mean.data(),
                                 f.guides[i], hin.data(), nullptr, cam, true);
      CHECK(o.n == 4 && o.changed && same_bytes(got[i], var[i], o.rec, o.var), "2x2: pixel %zu has n = %d", i, o.n);
      for (int k = 0; k < 3; ++k) CHECK(got[i].mean[k] < 2.0f && plain[i].mean[k] > 8.0f, "2x2: pixel %zu is clamped (%g, unclamped %g)", i, got[i].mean[k], plain[i].mean[k]);
    }
  }
  {  // a window of nine NaN pixels: n = 0, the history's bytes are the unclamped call's
    const float v[3] = {0.5f, 0.25f, 0.75f}, far[3] = {10.0f, 10.0f, 10.0f};
    Frame f = constant_frame(5, 5, v);
    for (int y = 1; y <= 3; ++y)
      for (int x = 1; x <= 3; ++x) f.mean[3 * (y * 5 + x) + (x + y) % 3] = NAN;
    const std::vector<History> hin = constant_history(25, far, 8.0f);
    run(f, P, &K, &hin, cam, true, got, var);
    run(f, P, nullptr, &hin, cam, true, plain, plain_var);
    const size_t c = 2 * 5 + 2;
    CHECK(same_bytes(got[c], var[c], plain[c], plain_var[c]), "nine NaN pixels: the history was clamped all the same");
    f.mean[3 * c] = f.mean[3 * c + 1] = f.mean[3 * c + 2] = 0.5f;  // the same nine, finite: the clamp was there to bite
    for (int y = 1; y <= 3; ++y)
      for (int x = 1; x <= 3; ++x) f.mean[3 * (y * 5 + x) + (x + y) % 3] = 0.5f;
    run(f, P, &K, &hin, cam, true, got, var);
    CHECK(got[c].mean[0] == 0.5f && plain[c].mean[0] > 8.0f, "nine finite pixels: %g (unclamped %g)", got[c].mean[0], plain[c].mean[0]);
  }
  {  // a NaN neighbour is a neighbour outside the image: column 0 of a 4x4 image against column 1 of a 5x4 one
    const float zero[3] = {0, 0, 0};
    Frame a = constant_frame(4, 4, zero), b = constant_frame(5, 4, zero);
    std::vector<History> ha = constant_history(16, zero, 8.0f), hb = constant_history(20, zero, 8.0f);
    for (int y = 0; y < 4; ++y)
      for (int x = 0; x < 4; ++x) {
        for (int k = 0; k < 3; ++k) {
          a.mean[3 * (y * 4 + x) + k] = b.mean[3 * (y * 5 + x + 1) + k] = (float)rnd(0, 1);
          ha[y * 4 + x].mean[k] = hb[y * 5 + x + 1].mean[k] = (float)rnd(0, 3);
        }
      }
    for (int y = 0; y < 4; ++y) b.mean[3 * (y * 5) + y % 3] = y & 1 ? NAN : INFINITY;
    std::vector<History> gb;
    std::vector<float> vb;
    run(a, P, &K, &ha, cam, true, got, var);
    run(b, P, &K, &hb, cam, true, gb, vb);
    long changed = 0;
    for (int y = 0; y < 4; ++y)
      for (int x = 0; x < 4; ++x) {
        CHECK(same_bytes(got[y * 4 + x], var[y * 4 + x], gb[y * 5 + x + 1], vb[y * 5 + x + 1]), "a NaN neighbour at (%d, %d) is not a missing one", x, y);
        changed += got[y * 4 + x].mean[0] != (float)((double)ha[y * 4 + x].mean[0] + (1.0 / 9.0) * ((double)a.mean[3 * (y * 4 + x)] - (double)ha[y * 4 + x].mean[0]));
      }
    CHECK(changed >= 4, "the shifted images: the clamp bites (%ld pixels)", changed);
  }
}

// Noise and lag together: a smooth 64x48 image under iid Gaussian noise of sigma 0.1, static camera, gamma 1, r 1.
static double rmse(const std::vector<History>& h, const std::vector<float>& truth) {
  double s = 0;
  for (size_t i = 0; i < h.size(); ++i)
    for (int k = 0; k < 3; ++k) s += ((double)h[i].mean[k] - truth[3 * i + k]) * ((double)h[i].mean[k] - truth[3 * i + k]);
  return std::sqrt(s / (3.0 * (double)h.size()));
}
static void noise_and_lag() {
  const int W = 64, H = 48, K0 = 16;
  const size_t n = (size_t)W * H;
  std::vector<float> truth(3 * n), turned(3 * n);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      float* t = &truth[3 * ((size_t)y * W + x)];
      t[0] = (float)(0.5 + 0.3 * std::sin(6.283185307179586 * (x + 0.5) / W));
      t[1] = (float)(0.5 + 0.3 * std::sin(6.283185307179586 * (y + 0.5) / H));
      t[2] = (float)(0.4 + 0.2 * x / (W - 1) + 0.1 * y / (H - 1));
    }
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) turned[3 * i + k] = truth[3 * (n - 1 - i) + k];  // the 180-degree rotation
  const float zero[3] = {0, 0, 0};
  Frame f = constant_frame(W, H, zero);
  const Cam cam = look_cam(13, 2, 3, (double)W / H);
  rtwt::Params P;
  CHECK(rtwt::resolve(0, 0, 0, 0, P), "resolve");
  const rtwt::Clamp K{1.0, 1};
  std::vector<History> hc[2], hu[2];
  std::vector<float> var;
  double in_rmse = 0;
  auto frame = [&](int k, const std::vector<float>& t) {
    double s = 0;
    for (size_t j = 0; j < 3 * n; ++j) {
      f.mean[j] = (float)(t[j] + 0.1 * gauss());
      s += ((double)f.mean[j] - t[j]) * ((double)f.mean[j] - t[j]);
    }
    in_rmse = std::sqrt(s / (3.0 * (double)n));
    run(f, P, &K, k ? &hc[(k + 1) & 1] : nullptr, cam, true, hc[k & 1], var);
    run(f, P, nullptr, k ? &hu[(k + 1) & 1] : nullptr, cam, true, hu[k & 1], var);
  };
  for (int k = 0; k < K0; ++k) frame(k, truth);
  const double still_c = rmse(hc[(K0 - 1) & 1], truth) / in_rmse, still_u = rmse(hu[(K0 - 1) & 1], truth) / in_rmse;
  std::printf("noise and lag: still image after %d frames: clamped %.3fx the input's RMSE (%.4f), unclamped %.3fx\n", K0, still_c, in_rmse, still_u);
  CHECK(still_c <= 0.35, "still image: the clamped mean is at %.3fx its input's RMSE", still_c);
  for (int k = K0; k < K0 + 2; ++k) frame(k, turned);
  const double lag_c = rmse(hc[(K0 + 1) & 1], turned) / in_rmse, lag_u = rmse(hu[(K0 + 1) & 1], turned) / in_rmse;
  std::printf("noise and lag: two frames after the image turned: clamped %.3fx, unclamped %.3fx\n", lag_c, lag_u);
  CHECK(lag_c < 1.0, "after the change: the clamped mean is at %.3fx its input's RMSE", lag_c);
  CHECK(lag_u > 1.5, "after the change: the unclamped mean is at %.3fx only: the case does not lag", lag_u);
}

static void option_ranges() {
  rtwt::Clamp K;
  CHECK(rtwt::resolve_clamp(0, 0, 0, K) && K.gamma == rtwt::kDefClampGamma && K.radius == 1, "defaults");
  CHECK(rtwt::resolve_clamp(2.5, 3, 0, K) && K.gamma == 2.5 && K.radius == 3, "gamma 2.5, radius 3");
  CHECK(rtwt::resolve_clamp(9.99e29, 1, 0, K), "gamma below 1e30");
  CHECK(!rtwt::resolve_clamp(-0.5, 0, 0, K) && !rtwt::resolve_clamp(NAN, 0, 0, K) && !rtwt::resolve_clamp(INFINITY, 0, 0, K) &&
            !rtwt::resolve_clamp(1e30, 0, 0, K) && !rtwt::resolve_clamp(1, 4, 0, K) && !rtwt::resolve_clamp(1, 0, 1, K),
        "option ranges");
}

int main() {
  second_statement_and_containment();
  identity();
  step_change();
  borders_and_skips();
  noise_and_lag();
  option_ranges();
  std::printf("temporal_clamp_check: bad %d/%d\n", g_bad, g_checks);
  return g_bad ? 1 : 0;
}
