// Device check of the Tier-B contract's building blocks: the gfx950 build of
// csrc/rtw_libm.hpp, rtw_math.hpp's sin_sign / checker_odd and f32 div_rn, the
// device's own f32 1/b and sqrt, and rtw_device.hpp's RNG (sm_mix, rnd_f64,
// rnd_f32, rnd3, f64_long_lz with their rare branches), each evaluated on the
// GPU over host-generated inputs and compared HERE, on the host, bit for bit
// with the oracle's C code (oracle/ro_libm.h, oracle/rtw_oracle.c) or plain
// IEEE host arithmetic — never with a host build of the header under test.
// Two NaNs count as equal (contract_compare.hpp).
//
// Prints one line per family, "family <name> cases N mismatches M", then the
// first mismatching inputs in hex; exit status 1 on any mismatch.  sin / cos
// with |x| >= 2^20 * pi/2 are outside the contract (the device returns ocml's
// value, the oracle glibc's): that family ("payne_hanek") is counted and
// printed with its largest ulp distance, and asserts nothing.
// "f64_long_lz state 0x... lz N" lines are for tests/test_gpu_contract.py,
// which restates the oracle's loop in Python.
//
// Limit: inlined code in this translation unit can compile differently from
// the same code inside world_kernel (as for gpu_math_check);
// tests/test_gpu_world_textures.py is the end-to-end counterpart.
// Built by the package Makefile (bin/gpu_contract_check); run by
// tests/test_gpu_contract.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "contract_compare.hpp"
#include "libm_inputs.hpp"
#include "ro_libm.h"
#include "rtw_device.hpp"
#include "rtw_libm.hpp"
#include "rtw_math.hpp"
#include "rtw_oracle.h"

#define HIP_OK(e)                                                                         \
  do {                                                                                    \
    const hipError_t err_ = (e);                                                          \
    if (err_ != hipSuccess) {                                                             \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(err_));   \
      std::exit(2);                                                                       \
    }                                                                                     \
  } while (0)

// ------------------------------------------------------------- kernels ----
#define GRID_STRIDE(i, n) \
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (n); i += (size_t)gridDim.x * blockDim.x)

__global__ void k_sincos(const double* x, size_t n, double* s, double* c) {
  GRID_STRIDE(i, n) {
    s[i] = rtwl::sin(x[i]);
    c[i] = rtwl::cos(x[i]);
  }
}
__global__ void k_atan2(const double* y, const double* x, size_t n, double* o) {
  GRID_STRIDE(i, n) o[i] = rtwl::atan2(y[i], x[i]);
}
__global__ void k_acos(const double* c, size_t n, double* o) {
  GRID_STRIDE(i, n) o[i] = rtwl::acos(c[i]);
}
__global__ void k_sin_sign(const double* a, size_t n, int32_t* o) {
  GRID_STRIDE(i, n) o[i] = rtwm::sin_sign(a[i]);
}
__global__ void k_checker(const double* a, size_t n, int32_t* o) {  // n triples
  GRID_STRIDE(i, n) o[i] = rtwm::checker_odd(a[3 * i], a[3 * i + 1], a[3 * i + 2]) ? 1 : 0;
}
__global__ void k_f32(const float* x, const float* b, const float* y_host, size_t n, float* q_hy, float* q_dy, float* y_dev,
                      float* sq) {
  GRID_STRIDE(i, n) {
    const float yd = 1.0f / b[i];
    y_dev[i] = yd;
    q_hy[i] = rtwm::div_rn(x[i], b[i], y_host[i]);
    q_dy[i] = rtwm::div_rn(x[i], b[i], yd);
    sq[i] = sqrt(x[i]);
  }
}
__global__ void k_mix(const uint64_t* z, size_t n, uint64_t* o) {
  GRID_STRIDE(i, n) o[i] = rtwk::sm_mix(z[i]);
}
constexpr int kDraws = 4;  // consecutive rnd draws per state
__global__ void k_rng(const uint64_t* st, size_t n, double* d64, uint64_t* s64, float* d32, uint64_t* s32, double* t64,
                      uint64_t* t64s, float* t32, uint64_t* t32s) {
  GRID_STRIDE(i, n) {
    uint64_t s = st[i];
    for (int k = 0; k < kDraws; ++k) {
      d64[kDraws * i + k] = rtwk::rnd_f64(s);
      s64[kDraws * i + k] = s;
    }
    s = st[i];
    for (int k = 0; k < kDraws; ++k) {
      d32[kDraws * i + k] = rtwk::rnd_f32(s);
      s32[kDraws * i + k] = s;
    }
    double a, b, c;
    uint64_t s2;
    rtwk::rnd3<double>(st[i], a, b, c, s2);
    t64[3 * i] = a, t64[3 * i + 1] = b, t64[3 * i + 2] = c;
    t64s[i] = s2;
    float fa, fb, fc;
    rtwk::rnd3<float>(st[i], fa, fb, fc, s2);
    t32[3 * i] = fa, t32[3 * i + 1] = fb, t32[3 * i + 2] = fc;
    t32s[i] = s2;
  }
}
__global__ void k_long_lz(const uint64_t* d, size_t n, uint32_t* o) {
  GRID_STRIDE(i, n) o[i] = rtwk::f64_long_lz(d[i]);
}

// --------------------------------------------------------- host helpers ----
template <typename T>
struct Dev {  // a device array, optionally initialised from the host
  T* p = nullptr;
  size_t n;
  explicit Dev(size_t n_) : n(n_) { HIP_OK(hipMalloc(&p, sizeof(T) * (n ? n : 1))); }
  explicit Dev(const std::vector<T>& h) : Dev(h.size()) {
    if (n) HIP_OK(hipMemcpy(p, h.data(), sizeof(T) * n, hipMemcpyHostToDevice));
  }
  ~Dev() { (void)hipFree(p); }
  std::vector<T> get() const {
    std::vector<T> h(n);
    if (n) HIP_OK(hipMemcpy(h.data(), p, sizeof(T) * n, hipMemcpyDeviceToHost));
    return h;
  }
};
#define LAUNCH(k, ...)                                                  \
  do {                                                                  \
    hipLaunchKernelGGL(k, dim3(1024), dim3(256), 0, 0, __VA_ARGS__);    \
    HIP_OK(hipGetLastError());                                          \
    HIP_OK(hipDeviceSynchronize());                                     \
  } while (0)

static uint64_t splitmix(uint64_t& s) {  // input generator only
  uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
static float f32_from(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
static int sign_of(double s) { return (s > 0) - (s < 0); }

constexpr uint64_t kGammaH = 0x9e3779b97f4a7c15ULL, kExtH = 0x5851F42D4C957F2DULL;
// inverse of ro_tb_mix (four Feistel half-rounds; as tests/test_oracle_kat.py's unmix)
static uint64_t unmix(uint64_t z) {
  static const uint32_t M[4] = {0xD2511F53u, 0xCD9E8D57u, 0x9E3779B1u, 0x85EBCA6Bu};
  uint32_t hi = (uint32_t)(z >> 32), lo = (uint32_t)z;
  for (int i = 3; i >= 0; --i) {
    uint32_t inv = M[i];  // Newton: inv * M == 1 mod 2^32
    for (int k = 0; k < 5; ++k) inv *= 2u - M[i] * inv;
    if (i % 2 == 0) {
      const uint32_t h0 = hi * inv;
      lo ^= (uint32_t)(((uint64_t)h0 * M[i]) >> 32);
      hi = h0;
    } else {
      const uint32_t l0 = lo * inv;
      hi ^= (uint32_t)(((uint64_t)l0 * M[i]) >> 32);
      lo = l0;
    }
  }
  return ((uint64_t)hi << 32) | lo;
}
static uint32_t clz64h(uint64_t v) { return v ? (uint32_t)__builtin_clzll(v) : 64u; }
// the loop of ro_sm_f64 (oracle/rtw_oracle.c) for a draw at Weyl state `draw_state`
static uint32_t long_lz_ref(uint64_t draw_state) {
  uint64_t ext = draw_state ^ kExtH;
  uint64_t lz = 12;
  for (;;) {
    ext += kGammaH;
    const uint64_t addl = clz64h(ro_tb_mix(ext));
    lz += addl;
    if (addl != 64) break;
    if (lz >= 1022) {
      lz = 1022;
      break;
    }
  }
  return (uint32_t)lz;
}

static int failed = 0;
static void finish(const cc::Family& f) {
  f.print();
  if (f.mismatches) failed = 1;
}

// ---------------------------------------------------------------- libm ----
static void check_libm(long n_random) {
  const std::vector<double> xs = libm_inputs(n_random, 7);
  std::vector<double> ay(xs.size()), ac(xs.size());
  for (size_t i = 0; i < xs.size(); ++i) {
    ay[i] = libm_atan2_partner(xs, i);
    ac[i] = libm_acos_arg(xs[i]);
  }
  std::vector<double> ey, ex, ec;
  sphere_uv_edges(ey, ex, ec);
  // Payne-Hanek range, for the count only: every binade from 2^21 up, both signs
  std::vector<double> ph;
  uint64_t g = 99;
  for (int i = 0; i < 200000; ++i) {
    const uint64_t z = splitmix(g);
    const uint64_t e = 1023 + 21 + (z >> 52) % (1023 - 21);
    double x;
    const uint64_t u = (z & 0x800FFFFFFFFFFFFFULL) | (e << 52);
    std::memcpy(&x, &u, 8);
    ph.push_back(x);
  }
  std::vector<double> sx = xs;
  sx.insert(sx.end(), ph.begin(), ph.end());
  {
    Dev<double> dx(sx), ds(sx.size()), dc(sx.size());
    LAUNCH(k_sincos, dx.p, sx.size(), ds.p, dc.p);
    const std::vector<double> s = ds.get(), c = dc.get();
    cc::Family fs("libm_sin"), fc("libm_cos");
    uint64_t ph_cases = 0, ph_diff = 0, ph_maxulp = 0;
    for (size_t i = 0; i < sx.size(); ++i) {
      const double x = sx[i];
      if (libm_payne_hanek(x)) {  // outside the contract: count, assert nothing
        for (int k = 0; k < 2; ++k) {
          const double got = k ? c[i] : s[i], ref = k ? ro_cos(x) : ro_sin(x);
          ++ph_cases;
          if (!cc::same(got, ref)) ++ph_diff;
          const uint64_t u = cc::ulp_distance(got, ref);
          if (u > ph_maxulp) ph_maxulp = u;
        }
        continue;
      }
      fs.check(i, cc::bits(x), 0, s[i], ro_sin(x));
      fc.check(i, cc::bits(x), 0, c[i], ro_cos(x));
    }
    finish(fs);
    finish(fc);
    std::printf("family payne_hanek cases %llu differing %llu max_ulp %llu (outside the contract: not asserted)\n",
                (unsigned long long)ph_cases, (unsigned long long)ph_diff, (unsigned long long)ph_maxulp);
  }
  {
    std::vector<double> y = ay, x = xs;
    y.insert(y.end(), ey.begin(), ey.end());
    x.insert(x.end(), ex.begin(), ex.end());
    Dev<double> dy(y), dx(x), dout(x.size());
    LAUNCH(k_atan2, dy.p, dx.p, x.size(), dout.p);
    const std::vector<double> o = dout.get();
    cc::Family f("libm_atan2");
    for (size_t i = 0; i < x.size(); ++i) f.check(i, cc::bits(y[i]), cc::bits(x[i]), o[i], ro_atan2(y[i], x[i]));
    finish(f);
  }
  {
    std::vector<double> c = ac;
    c.insert(c.end(), ec.begin(), ec.end());
    Dev<double> dc(c), dout(c.size());
    LAUNCH(k_acos, dc.p, c.size(), dout.p);
    const std::vector<double> o = dout.get();
    cc::Family f("libm_acos");
    for (size_t i = 0; i < c.size(); ++i) f.check(i, cc::bits(c[i]), 0, o[i], ro_acos(c[i]));
    finish(f);
  }
}

// ------------------------------------------------ sin_sign / checker_odd ----
static void check_sin_sign() {
  std::vector<double> a;
  const long double pil = 3.14159265358979323846264338327950288L;
  for (long k = 1; (double)(k * pil) < 524288.0; ++k) {  // the three doubles around every k * pi
    const double m = (double)(k * pil);
    for (double v : {std::nextafter(m, 0.0), m, std::nextafter(m, 1e300)}) {
      if (!(v < 524288.0)) continue;
      a.push_back(v);
      a.push_back(-v);
    }
  }
  const size_t n_kpi = a.size();
  uint64_t g = 5;
  for (int i = 0; i < 300000; ++i) {  // 10 * p for points of scene magnitudes (|p| from 1e-3 to ~3e3)
    const uint64_t z = splitmix(g);
    const double u = (double)(z >> 11) * 0x1p-53, e = (double)(splitmix(g) >> 11) * 0x1p-53;
    a.push_back(10.0 * ((2.0 * u - 1.0) * std::pow(10.0, -3.0 + 6.5 * e)));
  }
  for (double v : {0.0, -0.0, 5e-324, -5e-324, 0x1p-1022, 524287.99999999994, -524287.99999999994}) a.push_back(v);
  // [2^19, 2^20 * pi/2): the device falls back to ocml's sin, the oracle is still the musl algorithm
  const double top = 0x1p20 * 1.57079632679489661923;
  for (int i = 0; i < 200000; ++i) {
    const double u = (double)(splitmix(g) >> 11) * 0x1p-53;
    const double v = 524288.0 + u * (top - 524288.0);
    if (libm_payne_hanek(v)) continue;
    a.push_back(i & 1 ? -v : v);
  }
  for (double v : {524288.0, -524288.0, std::nextafter(524288.0, 1e300)}) a.push_back(v);
  for (long k = 166887; k < 333772; k += 97) {  // and the doubles around k * pi there
    const double m = (double)(k * pil);
    for (double v : {std::nextafter(m, 0.0), m, std::nextafter(m, 1e300)})
      if (v >= 524288.0 && !libm_payne_hanek(v)) a.push_back(v), a.push_back(-v);
  }
  while (a.size() % 3) a.push_back(1.0);
  Dev<double> da(a);
  Dev<int32_t> ds(a.size()), dodd(a.size() / 3);
  LAUNCH(k_sin_sign, da.p, a.size(), ds.p);
  LAUNCH(k_checker, da.p, a.size() / 3, dodd.p);
  const std::vector<int32_t> s = ds.get(), odd = dodd.get();
  cc::Family f("sin_sign"), fo("checker_odd");
  uint64_t underflowed = 0;
  for (size_t i = 0; i < a.size(); ++i) f.check(i, cc::bits(a[i]), 0, s[i], (int32_t)sign_of(ro_sin(a[i])));
  for (size_t i = 0; i < a.size() / 3; ++i) {
    // texture.zig:80 tests sin * sin * sin < 0; the kernel decides by the three signs.  The two agree
    // unless the product underflows to +-0 (|product| < 2^-1075: a hit within ~1e-108 of the origin on
    // all three axes; rtw_math.hpp states this limit), so the signs are what is compared here
    const int sp = sign_of(ro_sin(a[3 * i])) * sign_of(ro_sin(a[3 * i + 1])) * sign_of(ro_sin(a[3 * i + 2]));
    const double prod = ro_sin(a[3 * i]) * ro_sin(a[3 * i + 1]) * ro_sin(a[3 * i + 2]);
    if ((prod < 0) != (sp < 0)) ++underflowed;
    fo.check(i, cc::bits(a[3 * i]), cc::bits(a[3 * i + 1]), odd[i], (int32_t)(sp < 0 ? 1 : 0));
  }
  std::printf("checker_odd: %llu triples whose product of sines underflows to zero (decided by sign)\n",
              (unsigned long long)underflowed);
  std::printf("sin_sign inputs: %zu around k*pi, %zu in all\n", n_kpi, a.size());
  finish(f);
  finish(fo);
}

// ------------------------------------------------------- f32 arithmetic ----
static void check_f32(size_t n) {
  std::vector<float> x(n), b(n), y(n);
  uint64_t g = 0x243F6A8885A308D3ULL;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t z = splitmix(g), w = splitmix(g);
    const uint32_t man = (uint32_t)z & 0x007FFFFFu, wman = (uint32_t)w & 0x007FFFFFu, sgn = (uint32_t)(w >> 32) & 0x80000000u;
    const uint32_t e60 = 127 - 60 + (uint32_t)((z >> 32) % 121), f60 = 127 - 60 + (uint32_t)((w >> 33) % 121);
    uint32_t xb, bb = man | (e60 << 23);
    switch (i % 8) {
      case 0:  // any bit pattern (zeros, subnormals, inf, NaN; negative: sqrt gives NaN)
        xb = (uint32_t)(w >> 16);
        if (i % 16) xb &= 0x7FFFFFFFu;
        break;
      case 1:  // exponents in +-60, both signs
        xb = sgn | wman | (f60 << 23);
        break;
      case 2: {  // perfect squares (12-bit r: r * r is exact) and their neighbours
        const float r = f32_from((wman & 0x007FF800u) | (127u << 23));
        float s = r * r;
        std::memcpy(&xb, &s, 4);
        xb = xb + ((uint32_t)(z >> 60) & 7u) - 3u + (((uint32_t)(w >> 40) % 60u) << 23);
        break;
      }
      case 3:  // near-all-ones mantissas in x and b
        xb = sgn | ((0x007FFFFFu - ((uint32_t)(w >> 60) & 3u)) | (f60 << 23));
        bb = (bb | 0x007FFFFFu) - ((uint32_t)(z >> 61) & 3u);
        break;
      case 4: {  // quotients around div_rn's 2^120 and 2^-100 fall-back thresholds
        const bool up = (w >> 50) & 1;
        const int eb = (up ? -60 : -25) + (int)((z >> 32) % 61);  // b's exponent: [-60, 0] or [-25, 35]
        const int ex = eb + (up ? 120 : -100) + (int)((w >> 52) % 3) - 1;  // x's: [59, 121] or [-126, -64]
        bb = man | ((uint32_t)(127 + eb) << 23);
        xb = sgn | wman | ((uint32_t)(127 + ex) << 23);
        break;
      }
      case 5:  // subnormal x, b of any small exponent
        xb = sgn | wman;
        bb = man | ((uint32_t)((z >> 32) % 128) << 23);
        break;
      case 6:  // subnormal b
        xb = sgn | wman | ((uint32_t)((w >> 33) % 60) << 23);
        bb = man;
        break;
      default:  // tiny and huge normals on both sides
        xb = sgn | wman | ((uint32_t)(((w >> 33) & 1) ? 1 + (w >> 34) % 40 : 215 + (w >> 34) % 40) << 23);
        bb = man | ((uint32_t)(((z >> 33) & 1) ? 1 + (z >> 34) % 40 : 215 + (z >> 34) % 40) << 23);
    }
    if ((z >> 59) == 0) bb |= 0x80000000u;
    x[i] = f32_from(xb);
    b[i] = f32_from(bb);
    y[i] = 1.0f / b[i];
  }
  Dev<float> dx(x), db(b), dy(y), q1(n), q2(n), yd(n), sq(n);
  LAUNCH(k_f32, dx.p, db.p, dy.p, n, q1.p, q2.p, yd.p, sq.p);
  const std::vector<float> hq1 = q1.get(), hq2 = q2.get(), hyd = yd.get(), hsq = sq.get();
  cc::Family f1("f32_div_rn_host_y"), f2("f32_div_rn_device_y"), f3("f32_device_rcp"), f4("f32_device_sqrt");
  for (size_t i = 0; i < n; ++i) {
    const float q = x[i] / b[i];
    f1.check(i, cc::bits(x[i]), cc::bits(b[i]), hq1[i], q);
    f2.check(i, cc::bits(x[i]), cc::bits(b[i]), hq2[i], q);
    f3.check(i, cc::bits(b[i]), 0, hyd[i], y[i]);
    f4.check(i, cc::bits(x[i]), 0, hsq[i], sqrtf(x[i]));
  }
  finish(f1);
  finish(f2);
  finish(f3);
  finish(f4);
}

// ------------------------------------------------------------------ RNG ----
static void check_rng(size_t n_random) {
  {  // the mixer: the known-answer inputs of tests/golden/rng_kat.json (tb_mix_in) and random words
    std::vector<uint64_t> z = {0ULL, 1ULL, 4294967296ULL, 11400714819323198485ULL, 18446744073709551615ULL,
                               7259720743724543637ULL};  // tb_mix_in; the test compares the lines below with tb_mix_out
    const size_t n_kat = z.size();
    uint64_t g = 11;
    for (size_t i = 0; i < n_random; ++i) z.push_back(splitmix(g));
    Dev<uint64_t> dz(z), dout(z.size());
    LAUNCH(k_mix, dz.p, z.size(), dout.p);
    const std::vector<uint64_t> o = dout.get();
    cc::Family f("rng_sm_mix");
    for (size_t i = 0; i < z.size(); ++i) f.check(i, z[i], 0, o[i], ro_tb_mix(z[i]));
    for (size_t i = 0; i < n_kat; ++i) std::printf("sm_mix %llu -> %llu\n", (unsigned long long)z[i], (unsigned long long)o[i]);
    finish(f);
  }
  std::vector<uint64_t> st;
  uint64_t g = 3;
  const uint64_t seeds[] = {0ULL, 42ULL, 0xFFFFFFFFFFFFFFFFULL, 0x100000005ULL};
  const uint64_t pixels[] = {0ULL, 1ULL, 8294399ULL};
  const uint64_t samples[] = {0ULL, 1ULL, (1ULL << 24) - 1};
  for (uint64_t sd : seeds)
    for (uint64_t px : pixels)
      for (uint64_t sm : samples) st.push_back(ro_tierb_state(sd, px, sm));
  for (size_t i = 0; i < n_random; ++i) {
    const uint64_t sd = splitmix(g), px = splitmix(g) % 8294400ULL, sm = splitmix(g) >> 40;
    st.push_back(ro_tierb_state(sd, px, sm));
  }
  // constructed states unmix(v) - k * gamma: the word with >= 12 (f64) / >= 41 (f32) leading zeros is
  // draw k, so it lands in each of rnd3's three slots and in plain rnd
  cc::Family fb("rng_branch_taken");
  const size_t first_constructed = st.size();
  for (int f32 = 0; f32 < 2; ++f32) {
    const int bits = f32 ? 23 : 52;
    std::vector<uint64_t> vs = {0ULL, 1ULL, 1ULL << (bits - 1), (1ULL << bits) - 1};
    for (int i = 0; i < 2000; ++i) vs.push_back(splitmix(g) >> (64 - bits));
    for (int i = 0; i < 64; ++i) vs.push_back(splitmix(g) >> (64 - bits + (i % bits)));  // every leading-zero count
    for (uint64_t v : vs)
      for (uint64_t k = 1; k <= 3; ++k) {
        const uint64_t s = unmix(v) - k * kGammaH;
        fb.check(st.size(), s, k, ro_tb_mix(s + k * kGammaH) >> bits, (uint64_t)0);  // the oracle takes the branch
        st.push_back(s);
      }
  }
  finish(fb);
  std::printf("rng states: %zu Tier-B, %zu constructed\n", first_constructed, st.size() - first_constructed);
  const size_t n = st.size();
  Dev<uint64_t> ds(st), s64(n * kDraws), s32(n * kDraws), t64s(n), t32s(n);
  Dev<double> d64(n * kDraws), t64(n * 3);
  Dev<float> d32(n * kDraws), t32(n * 3);
  LAUNCH(k_rng, ds.p, n, d64.p, s64.p, d32.p, s32.p, t64.p, t64s.p, t32.p, t32s.p);
  const std::vector<double> hd64 = d64.get(), ht64 = t64.get();
  const std::vector<float> hd32 = d32.get(), ht32 = t32.get();
  const std::vector<uint64_t> hs64 = s64.get(), hs32 = s32.get(), ht64s = t64s.get(), ht32s = t32s.get();
  cc::Family f64v("rng_rnd_f64"), f64s("rng_rnd_f64_state"), f32v("rng_rnd_f32"), f32s("rng_rnd_f32_state"),
      t64v("rng_rnd3_f64"), t64st("rng_rnd3_f64_s2"), t32v("rng_rnd3_f32"), t32st("rng_rnd3_f32_s2");
  for (size_t i = 0; i < n; ++i) {
    uint64_t s = st[i];
    for (int k = 0; k < kDraws; ++k) {
      const double want = ro_sm_f64(&s);
      f64v.check(i, st[i], k, hd64[kDraws * i + k], want);
      f64s.check(i, st[i], k, hs64[kDraws * i + k], s);
      if (k < 3) t64v.check(i, st[i], k, ht64[3 * i + k], want);
      if (k == 1) t64st.check(i, st[i], k, ht64s[i], s);
    }
    s = st[i];
    for (int k = 0; k < kDraws; ++k) {
      const float want = ro_sm_f32(&s);
      f32v.check(i, st[i], k, hd32[kDraws * i + k], want);
      f32s.check(i, st[i], k, hs32[kDraws * i + k], s);
      if (k < 3) t32v.check(i, st[i], k, ht32[3 * i + k], want);
      if (k == 1) t32st.check(i, st[i], k, ht32s[i], s);
    }
  }
  for (const cc::Family* f : {&f64v, &f64s, &f32v, &f32s, &t64v, &t64st, &t32v, &t32st}) finish(*f);
  {  // f64_long_lz directly; d[0]: the first extension word is zero, so the loop iterates
    std::vector<uint64_t> d = {(unmix(0) - kGammaH) ^ kExtH};
    for (int lz = 0; lz < 64; ++lz) d.push_back((unmix(splitmix(g) >> lz) - kGammaH) ^ kExtH);  // every count of the first word
    for (int i = 0; i < 4096; ++i) d.push_back(splitmix(g));
    Dev<uint64_t> dd(d);
    Dev<uint32_t> dout(d.size());
    LAUNCH(k_long_lz, dd.p, d.size(), dout.p);
    const std::vector<uint32_t> o = dout.get();
    cc::Family f("rng_f64_long_lz");
    for (size_t i = 0; i < d.size(); ++i) f.check(i, d[i], 0, o[i], long_lz_ref(d[i]));
    cc::Family it("rng_f64_long_lz_iterates");
    it.check(0, d[0], 0, ro_tb_mix((d[0] ^ kExtH) + kGammaH), (uint64_t)0);
    finish(it);
    finish(f);
    for (size_t i = 0; i < 4; ++i) std::printf("f64_long_lz state 0x%016llx lz %u\n", (unsigned long long)d[i], o[i]);
  }
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 300000;
  check_libm(n);
  check_sin_sign();
  check_f32((size_t)1 << 20);
  check_rng(200000);
  std::printf("%s\n", failed ? "FAILED" : "ok");
  return failed;
}
