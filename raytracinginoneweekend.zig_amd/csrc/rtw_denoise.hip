// rtw_denoise.hip — device side of the feature-guided denoiser (rtw_hip.h
// rtw_denoise_device, rtw_denoise_spatial_variance_device,
// rtw_accum_variance_device, rtw_accum_denoise_device).  The filter itself is rtw_denoise.hpp's filter_pixel, the
// function rtw_denoise_host runs: the kernels here only decide where a tap's
// records come from, so the device's bytes are the host's.
//
// One launch per level.  A workgroup is a tile of 64 x 4 pixels, a wave one row
// of 64 consecutive x: centre loads and stores are coalesced, and every tap
// reads whole 16-byte records (colour + variance one dwordx4, the guide two).
//   direct form: a tap reads global memory (the working set, 48 B per pixel,
//                stays in L2 / the Infinity Cache between levels);
//   tiled form:  tap spacing S = 1 or 2 — the tile's footprint with its halo
//                of 2 S pixels, (64 + 4 S) x (4 + 4 S) records, is staged in LDS
//                first (S = 2: 864 records, 40.5 KiB); a cell outside the image
//                is staged as an empty pixel, which filter_pixel drops as it
//                drops the out-of-image tap.  Wider spacings do not fit.
// Which form runs a level: kTiledMaxStep, chosen by the A/B in DESIGN.md §14.
// The first level reads the caller's mean (3 floats) and variance, the last one
// writes the caller's mean and rgb8; the levels between ping-pong in the
// workspace.  With RTW_DENOISE_SPATIAL_VAR one launch of spatial_variance_kernel
// precedes the levels (§14.6); its map lives in the second workspace image,
// which no level writes before the second.  No atomics, no state.
// -ffp-contract=off (Makefile).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rtw_adaptive.hpp"
#include "rtw_capi_shared.hpp"
#include "rtw_denoise.hpp"

namespace rtwk {

namespace {

using rtwd::Guide;
using rtwd::Px;

constexpr int kDnTileW = 64, kDnTileH = 4;  // a wave = one row of the tile
constexpr int kDnBlock = kDnTileW * kDnTileH;
// Levels of tap spacing <= this run the tiled form (0: none).
#ifndef RTW_DENOISE_TILED_MAX_STEP
#define RTW_DENOISE_TILED_MAX_STEP 2
#endif
constexpr int kTiledMaxStep = RTW_DENOISE_TILED_MAX_STEP;

struct DenoiseArgs {
  const float* mean;  // first level: the caller's image
  const float* var;   // first level: optional
  const Px* in;       // later levels (null at the first)
  const Guide* guides;
  Px* out;            // every level but the last
  float* mean_out;    // last level (each optional)
  uint8_t* rgb_out;
  int W, H, step, last;
  rtwd::Params P;
};

__device__ __forceinline__ Px load_px(const DenoiseArgs& A, size_t i) {
  if (A.in) return A.in[i];  // (uniform)
  return Px{A.mean[3 * i], A.mean[3 * i + 1], A.mean[3 * i + 2], A.var ? A.var[i] : rtwd::kVarUnknown};
}

__device__ __forceinline__ void store_px(const DenoiseArgs& A, size_t i, const Px& r) {
  if (!A.last) {  // (uniform)
    A.out[i] = r;
    return;
  }
  if (A.mean_out) A.mean_out[3 * i] = r.r, A.mean_out[3 * i + 1] = r.g, A.mean_out[3 * i + 2] = r.b;
  if (A.rgb_out) {
    A.rgb_out[3 * i] = rtwd::quantise((double)r.r);
    A.rgb_out[3 * i + 1] = rtwd::quantise((double)r.g);
    A.rgb_out[3 * i + 2] = rtwd::quantise((double)r.b);
  }
}

// S = 0: the direct form; S = 1, 2: the tiled form for tap spacing S.
template <bool GUIDES, int S>
__global__ void __launch_bounds__(kDnBlock) denoise_level_kernel(DenoiseArgs A) {
  const int lx = (int)(threadIdx.x & (kDnTileW - 1)), ly = (int)(threadIdx.x >> 6);
  const int x0 = (int)blockIdx.x * kDnTileW, y0 = (int)blockIdx.y * kDnTileH;
  const int x = x0 + lx, y = y0 + ly;
  if constexpr (S == 0) {
    if (x >= A.W || y >= A.H) return;
    auto px = [&](int qx, int qy) { return load_px(A, (size_t)qy * A.W + qx); };
    auto gd = [&](int qx, int qy) { return A.guides[(size_t)qy * A.W + qx]; };
    const Px r = rtwd::filter_pixel<GUIDES>(x, y, A.W, A.H, A.step, A.P, px, gd);
    store_px(A, (size_t)y * A.W + x, r);
  } else {
    constexpr int TW = kDnTileW + 4 * S, TH = kDnTileH + 4 * S;
    __shared__ Px t_px[TW * TH];
    __shared__ Guide t_gd[GUIDES ? TW * TH : 1];
    const int tx0 = x0 - 2 * S, ty0 = y0 - 2 * S;
    for (int c = (int)threadIdx.x; c < TW * TH; c += kDnBlock) {
      const int cy = c / TW, cx = c - cy * TW;
      const int gx = tx0 + cx, gy = ty0 + cy;
      if (gx >= 0 && gx < A.W && gy >= 0 && gy < A.H) {
        const size_t i = (size_t)gy * A.W + gx;
        t_px[c] = load_px(A, i);
        if constexpr (GUIDES) t_gd[c] = A.guides[i];
      } else {  // outside the image: an empty pixel (never read as a tap: the filter checks the bounds first)
        t_px[c] = Px{0.0f, 0.0f, 0.0f, rtwd::kVarEmpty};
        if constexpr (GUIDES) t_gd[c] = Guide{};
      }
    }
    __syncthreads();
    if (x >= A.W || y >= A.H) return;
    auto px = [&](int qx, int qy) { return t_px[(qy - ty0) * TW + (qx - tx0)]; };
    auto gd = [&](int qx, int qy) { return t_gd[GUIDES ? (qy - ty0) * TW + (qx - tx0) : 0]; };
    const Px r = rtwd::filter_pixel<GUIDES>(x, y, A.W, A.H, S, A.P, px, gd);
    store_px(A, (size_t)y * A.W + x, r);
  }
}

template <bool GUIDES>
hipError_t launch_level(const DenoiseArgs& a, bool tiled, hipStream_t s) {
  const dim3 grid((a.W + kDnTileW - 1) / kDnTileW, (a.H + kDnTileH - 1) / kDnTileH), block(kDnBlock);
  if (tiled && a.step == 1)
    hipLaunchKernelGGL((denoise_level_kernel<GUIDES, 1>), grid, block, 0, s, a);
  else if (tiled && a.step == 2)
    hipLaunchKernelGGL((denoise_level_kernel<GUIDES, 2>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((denoise_level_kernel<GUIDES, 0>), grid, block, 0, s, a);
  return hipGetLastError();
}

// The spatial variance estimate (rtw_denoise.hpp spatial_variance_pixel) of every pixel.  The same
// 64 x 4 tile.  Tiled form: the tile's footprint with its halo of 3 pixels, 70 x 10 cells, is staged
// in LDS once — per cell the luminance as f64, the emptiness, and the guide as two 16-byte halves
// in two arrays: a row of lanes then reads consecutive 8- and 16-byte words, which ds_read_b64 /
// ds_read_b128 serve without a bank conflict (the 32-byte record read as two b128 halves would put
// lanes l and l + 8 of a 16-lane group on one slot: 2-way).  44 bytes x 700 cells = 30 800 bytes.
// A cell outside the image is staged as empty.  Direct form: every tap reads global memory.
struct SpatialArgs {
  const float* mean;
  const float* var;  // optional: null = all unknown
  const Guide* guides;
  float* out;
  int W, H;
  rtwd::Params P;
};

struct alignas(16) GuideHalf {
  float a, b, c;
  uint32_t d;  // (depth / prim as bits)
};

template <bool GUIDES, bool TILED>
__global__ void __launch_bounds__(kDnBlock) spatial_variance_kernel(SpatialArgs A) {
  const int lx = (int)(threadIdx.x & (kDnTileW - 1)), ly = (int)(threadIdx.x >> 6);
  const int x0 = (int)blockIdx.x * kDnTileW, y0 = (int)blockIdx.y * kDnTileH;
  const int x = x0 + lx, y = y0 + ly;
  auto load_tap = [&](size_t i) {
    return rtwd::sv_tap(Px{A.mean[3 * i], A.mean[3 * i + 1], A.mean[3 * i + 2], A.var ? A.var[i] : rtwd::kVarUnknown});
  };
  if constexpr (!TILED) {
    if (x >= A.W || y >= A.H) return;
    const size_t i = (size_t)y * A.W + x;
    auto tap = [&](int qx, int qy) { return load_tap((size_t)qy * A.W + qx); };
    auto gd = [&](int qx, int qy) { return A.guides[(size_t)qy * A.W + qx]; };
    const float vp = A.var ? A.var[i] : rtwd::kVarUnknown;
    A.out[i] = rtwd::spatial_variance_pixel<GUIDES>(x, y, A.W, A.H, A.P, vp, tap, gd);
  } else {
    constexpr int R = rtwd::kSpatialRadius;
    constexpr int TW = kDnTileW + 2 * R, TH = kDnTileH + 2 * R;
    __shared__ double t_y[TW * TH];
    __shared__ uint32_t t_e[TW * TH];
    __shared__ GuideHalf t_g0[GUIDES ? TW * TH : 1], t_g1[GUIDES ? TW * TH : 1];
    const int tx0 = x0 - R, ty0 = y0 - R;
    for (int c = (int)threadIdx.x; c < TW * TH; c += kDnBlock) {
      const int cy = c / TW, cx = c - cy * TW;
      const int gx = tx0 + cx, gy = ty0 + cy;
      if (gx >= 0 && gx < A.W && gy >= 0 && gy < A.H) {
        const size_t i = (size_t)gy * A.W + gx;
        const rtwd::SvTap t = load_tap(i);
        t_y[c] = t.y;
        t_e[c] = t.empty ? 1u : 0u;
        if constexpr (GUIDES) {
          const GuideHalf* g = reinterpret_cast<const GuideHalf*>(A.guides + i);
          t_g0[c] = g[0];
          t_g1[c] = g[1];
        }
      } else {  // outside the image: empty (never read as a tap: the estimate checks the bounds first)
        t_y[c] = 0.0;
        t_e[c] = 1u;
        if constexpr (GUIDES) t_g0[c] = GuideHalf{}, t_g1[c] = GuideHalf{};
      }
    }
    __syncthreads();
    if (x >= A.W || y >= A.H) return;
    const size_t i = (size_t)y * A.W + x;
    auto tap = [&](int qx, int qy) {
      const int c = (qy - ty0) * TW + (qx - tx0);
      return rtwd::SvTap{t_y[c], t_e[c] != 0u};
    };
    auto gd = [&](int qx, int qy) {
      const int c = GUIDES ? (qy - ty0) * TW + (qx - tx0) : 0;
      const GuideHalf h0 = t_g0[c], h1 = t_g1[c];
      return Guide{{h0.a, h0.b, h0.c}, __uint_as_float(h0.d), {h1.a, h1.b, h1.c}, h1.d};
    };
    const float vp = A.var ? A.var[i] : rtwd::kVarUnknown;
    A.out[i] = rtwd::spatial_variance_pixel<GUIDES>(x, y, A.W, A.H, A.P, vp, tap, gd);
  }
}

hipError_t launch_spatial(const SpatialArgs& a, hipStream_t s) {
  const dim3 grid((a.W + kDnTileW - 1) / kDnTileW, (a.H + kDnTileH - 1) / kDnTileH), block(kDnBlock);
  const bool tiled = !(a.P.flags & rtwd::kFlagDirect);
  if (a.guides) {
    if (tiled)
      hipLaunchKernelGGL((spatial_variance_kernel<true, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((spatial_variance_kernel<true, false>), grid, block, 0, s, a);
  } else {
    if (tiled)
      hipLaunchKernelGGL((spatial_variance_kernel<false, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((spatial_variance_kernel<false, false>), grid, block, 0, s, a);
  }
  return hipGetLastError();
}

// rtw_accum_variance_device: the squared standard error of the pixel's mean
// luminance (rtw_adaptive.hpp pixel_se2) as an f32, with the pixel's own count
// in the masked state (cnt), else `done`.
struct VarianceArgs {
  const double* stat;
  const uint32_t* cnt;  // masked state, else null
  float* var;
  uint32_t npix, done, chunk;
};
__global__ void __launch_bounds__(256) accum_variance_kernel(VarianceArgs V) {
  const double2* stat2 = reinterpret_cast<const double2*>(V.stat);
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < V.npix; i += gridDim.x * 256u) {
    const uint32_t n = V.cnt ? V.cnt[i] : V.done;
    const uint32_t m = n / V.chunk;
    float v = rtwd::kVarUnknown;
    if (n == 0u) {
      v = rtwd::kVarEmpty;
    } else if (m >= 2u) {
      const double2 y = stat2[i];
      v = (float)rtwa::pixel_se2(y.x, y.y, m, V.chunk);
    }
    V.var[i] = v;
  }
}

}  // namespace

}  // namespace rtwk

namespace {

int hip_fail(const char* what, hipError_t e) { return rtw_fail(RTW_EHIP, "%s: %s", what, hipGetErrorString(e)); }

// The levels of one call on stream s.  force_direct: every level in the direct form.
int run_levels(const float* d_mean, const float* d_var, const rtw_guide* d_guides, uint32_t W, uint32_t H,
               const rtwd::Params& P, void* workspace, uint8_t* d_rgb_out, float* d_mean_out, hipStream_t s) {
  using namespace rtwk;
  Px* buf[2] = {static_cast<Px*>(workspace),
                reinterpret_cast<Px*>(static_cast<unsigned char*>(workspace) + rtwd::image_bytes(W, H))};
  const bool force_direct = (P.flags & rtwd::kFlagDirect) != 0;
  if (P.flags & rtwd::kFlagSpatialVar) {  // the estimated map lives in the second image: level 1 only reads it
    float* est = reinterpret_cast<float*>(buf[1]);
    const hipError_t e = launch_spatial(SpatialArgs{d_mean, d_var, reinterpret_cast<const Guide*>(d_guides), est,
                                                    (int)W, (int)H, P}, s);
    if (e != hipSuccess) return hip_fail("spatial variance kernel launch", e);
    d_var = est;
  }
  for (uint32_t l = 0; l < P.levels; ++l) {
    DenoiseArgs a;
    a.mean = d_mean;
    a.var = d_var;
    a.in = l ? buf[(l - 1) & 1u] : nullptr;
    a.guides = reinterpret_cast<const Guide*>(d_guides);
    a.out = buf[l & 1u];
    a.mean_out = d_mean_out;
    a.rgb_out = d_rgb_out;
    a.W = (int)W, a.H = (int)H, a.step = 1 << l;
    a.last = l + 1 == P.levels;
    a.P = P;
    const bool tiled = !force_direct && a.step <= kTiledMaxStep;
    const hipError_t e = d_guides ? launch_level<true>(a, tiled, s) : launch_level<false>(a, tiled, s);
    if (e != hipSuccess) return hip_fail("denoise kernel launch", e);
  }
  return RTW_OK;
}

int accum_here(rtw_accum a, const char* who) {
  if (!a) return rtw_fail(RTW_EINVAL, "%s: accumulator is NULL", who);
  int dev = 0;
  const hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return hip_fail("hipGetDevice", e);
  if (dev != a->device)
    return rtw_fail(RTW_EINVAL, "%s: accumulator lives on device %d but the current device is %d", who, a->device, dev);
  return RTW_OK;
}

size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int rtw_denoise_device(const float* d_mean, const float* d_var, const rtw_guide* d_guides, uint32_t W, uint32_t H,
                       const rtw_denoise_opts* o, void* workspace, size_t workspace_bytes, uint8_t* d_rgb_out,
                       float* d_mean_out, void* stream) {
  const rtw_denoise_opts dflt{};
  if (!o) o = &dflt;
  rtwd::Params P;
  const int st = rtwd::check_call("rtw_denoise_device", d_mean, W, H, o->levels, o->sigma_color, o->sigma_normal,
                                  o->sigma_depth, o->sigma_albedo, o->flags, workspace, workspace_bytes, d_rgb_out,
                                  d_mean_out, P);
  if (st != RTW_OK) return st;
  if (((uintptr_t)d_guides & 15u) != 0) return rtw_fail(RTW_EINVAL, "rtw_denoise_device: d_guides is not 16-byte aligned");
  return run_levels(d_mean, d_var, d_guides, W, H, P, workspace, d_rgb_out, d_mean_out, static_cast<hipStream_t>(stream));
}

int rtw_denoise_spatial_variance_device(const float* d_mean, const float* d_var_in, const rtw_guide* d_guides, uint32_t W,
                                        uint32_t H, const rtw_denoise_opts* o, float* d_var_out, void* stream) {
  const rtw_denoise_opts dflt{};
  if (!o) o = &dflt;
  rtwd::Params P;
  const int st = rtwd::check_spatial_call("rtw_denoise_spatial_variance_device", d_mean, d_var_in, d_guides, W, H,
                                          o->levels, o->sigma_color, o->sigma_normal, o->sigma_depth, o->sigma_albedo,
                                          o->flags, d_var_out, P);
  if (st != RTW_OK) return st;
  if (((uintptr_t)d_guides & 15u) != 0)
    return rtw_fail(RTW_EINVAL, "rtw_denoise_spatial_variance_device: d_guides is not 16-byte aligned");
  const hipError_t e = rtwk::launch_spatial(
      rtwk::SpatialArgs{d_mean, d_var_in, reinterpret_cast<const rtwk::Guide*>(d_guides), d_var_out, (int)W, (int)H, P},
      static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail("spatial variance kernel launch", e);
  return RTW_OK;
}

int rtw_accum_variance_device(rtw_accum a, float* d_var, void* stream) {
  const int st = accum_here(a, "rtw_accum_variance_device");
  if (st != RTW_OK) return st;
  if (!d_var) return rtw_fail(RTW_EINVAL, "rtw_accum_variance_device: d_var is NULL");
  if (a->done == 0) return rtw_fail(RTW_EINVAL, "rtw_accum_variance_device: no sample accumulated yet");
  rtwk::VarianceArgs v;
  v.stat = a->stat;
  v.cnt = a->masked ? a->cnt : nullptr;
  v.var = d_var;
  v.npix = a->npix;
  v.done = a->done;
  v.chunk = a->chunk;
  const uint32_t grid = std::min((a->npix + 255u) / 256u, 2048u);
  hipLaunchKernelGGL(rtwk::accum_variance_kernel, dim3(grid ? grid : 1), dim3(256), 0, static_cast<hipStream_t>(stream), v);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("variance kernel launch", e);
  return RTW_OK;
}

// Workspace of rtw_accum_denoise_device: the filter's two images, then the
// resolved mean (npix x 3 f32), the variance (npix f32) and the resolve's rgb8.
size_t rtw_accum_denoise_workspace_bytes(rtw_accum a, const rtw_denoise_opts* o) {
  if (!a) {
    rtw_fail(RTW_EINVAL, "rtw_accum_denoise_workspace_bytes: accumulator is NULL");
    return 0;
  }
  const size_t f = rtw_denoise_workspace_bytes(a->p.width, a->p.row_count, o);
  if (f == 0) return 0;
  return f + al256((size_t)a->npix * 12) + al256((size_t)a->npix * 4) + al256((size_t)a->npix * 3);
}

int rtw_accum_denoise_device(rtw_accum a, const rtw_guide* d_guides, const rtw_denoise_opts* o, void* workspace,
                             size_t workspace_bytes, uint8_t* d_rgb, float* d_mean, void* stream) {
  int st = accum_here(a, "rtw_accum_denoise_device");
  if (st != RTW_OK) return st;
  if (a->p.row_stride != 1)
    return rtw_fail(RTW_UNSUPPORTED, "rtw_accum_denoise_device: row_stride %u: the filter needs contiguous image rows",
                    a->p.row_stride);
  if (a->done == 0) return rtw_fail(RTW_EINVAL, "rtw_accum_denoise_device: no sample accumulated yet");
  if (!workspace) return rtw_fail(RTW_EINVAL, "rtw_accum_denoise_device: workspace is NULL");
  const size_t need = rtw_accum_denoise_workspace_bytes(a, o);
  if (need == 0) return RTW_EINVAL;
  if (workspace_bytes < need)
    return rtw_fail(RTW_EINVAL, "rtw_accum_denoise_device: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  const uint32_t W = a->p.width, H = a->p.row_count;
  const size_t f = 2 * rtwd::image_bytes(W, H);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  float* mean = reinterpret_cast<float*>(ws + f);
  float* var = reinterpret_cast<float*>(ws + f + al256((size_t)a->npix * 12));
  uint8_t* rgb = ws + f + al256((size_t)a->npix * 12) + al256((size_t)a->npix * 4);
  st = rtw_accum_resolve_device(a, rgb, mean, stream);
  if (st != RTW_OK) return st;
  st = rtw_accum_variance_device(a, var, stream);
  if (st != RTW_OK) return st;
  return rtw_denoise_device(mean, var, d_guides, W, H, o, workspace, f, d_rgb, d_mean, stream);
}

}  // extern "C"
