// rtw_accum.hip — kernels of the progressive accumulator (rtw_hip.h
// rtw_accum_*): fold a pass's chunk sums into the frame's running f64 sum,
// resolve the sum to rgb8 / f32 mean, and estimate the frame's noise.
//
// Exactness: the fold adds the chunks of a pass to the pixel sum one by one,
// in chunk order, component by component — the additions finalize_kernel
// (rtw_trace.hip) makes over a one-shot render's chunks, in its order — and
// the resolve quantises with finalize_kernel's expression, so a frame
// accumulated over chunk-aligned passes has the one-shot frame's bytes
// (DESIGN.md §12).  -ffp-contract=off (Makefile): one IEEE operation per
// operator below.
#include <hip/hip_runtime.h>

#include "rtw_internal.hpp"

namespace rtwk {

namespace {

constexpr uint32_t kFoldBlock = 256;  // threads = pixels per tile
constexpr uint32_t kFoldTile = 3 * kFoldBlock;  // f64 values per tile

// One workgroup per tile of 256 pixels = 768 consecutive f64 values of `sum`
// and of every chunk of `partial`.  The sums are updated in that flat form:
// thread t owns values t, t + 256 and t + 512 of the tile, so every load and
// store of a wave covers 512 contiguous bytes.  The luminance statistic needs
// a pixel's three components together: the chunk's values pass through LDS
// (two buffers, one barrier per chunk) and thread t reads pixel t's triple.
__global__ void __launch_bounds__(kFoldBlock) accum_fold_kernel(FoldArgs F) {
  __shared__ double tile[2][kFoldTile];
  const uint32_t t = threadIdx.x;
  const size_t nflat = (size_t)F.npix * 3;
  const uint32_t n_tiles = (F.npix + kFoldBlock - 1) / kFoldBlock;
  double2* stat2 = reinterpret_cast<double2*>(F.stat);
  for (uint32_t ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
    const size_t base = (size_t)ti * kFoldTile + t;
    const uint32_t pix = ti * kFoldBlock + t;
    const bool pin = pix < F.npix;
    bool in[3];
    double s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      in[k] = base + k * kFoldBlock < nflat;
      s[k] = in[k] ? F.sum[base + k * kFoldBlock] : 0.0;
    }
    double2 y = make_double2(0.0, 0.0);
    if (pin && F.n_full) y = stat2[pix];
    for (uint32_t c = 0; c < F.n_chunks; ++c) {
      const double* P = F.partial + (size_t)c * nflat;
      double v[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        v[k] = in[k] ? P[base + k * kFoldBlock] : 0.0;
        s[k] += v[k];
      }
      if (c < F.n_full) {  // (uniform)
        double* T = tile[c & 1u];
#pragma unroll
        for (int k = 0; k < 3; ++k) T[t + k * kFoldBlock] = v[k];
        __syncthreads();
        if (pin) {
          const double r = T[3 * t], g = T[3 * t + 1], b = T[3 * t + 2];
          const double Y = (0.2126 * r + 0.7152 * g) + 0.0722 * b;
          y.x += Y;
          y.y += Y * Y;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (in[k]) F.sum[base + k * kFoldBlock] = s[k];
    if (pin && F.n_full) stat2[pix] = y;
    __syncthreads();  // the next tile's first chunk reuses tile[0]
  }
}

// finalize_kernel's quantisation (main.zig:395-400) of the running sum, value
// by value: the three components of a pixel are independent here.
__global__ void __launch_bounds__(256) accum_resolve_kernel(ResolveArgs F) {
  const size_t nflat = (size_t)F.npix * 3;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nflat; e += (size_t)gridDim.x * blockDim.x) {
    const double t = F.sum[e];
    const double g = sqrt(t * F.scale);
    const double cl = fmax(0.0, fmin(g, 0.999));
    F.rgb[e] = (uint8_t)(256.0 * cl);
    if (F.mean) F.mean[e] = (float)(t * F.scale);
  }
}

// Per pixel the squared standard error of the mean luminance, from the spread
// of the m full chunks' luminances: se2 = max(0, SY2 - SY SY / m) / (m (m-1) n_c^2).
// A fixed grid: thread g adds pixels g, g + G, ... in order, a workgroup adds
// its threads' sums in a fixed tree, accum_noise_last_kernel adds the
// workgroups' sums in index order — the same additions on every call.
__global__ void __launch_bounds__(256) accum_noise_kernel(NoiseArgs N) {
  __shared__ double red[256];
  const double2* stat2 = reinterpret_cast<const double2*>(N.stat);
  double acc = 0.0;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < N.npix; i += kNoiseGrid * 256u) {
    const double2 y = stat2[i];
    acc += fmax(0.0, y.y - y.x * y.x / N.m) / N.denom;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (uint32_t w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) N.part[blockIdx.x] = red[0];
}
__global__ void __launch_bounds__(64) accum_noise_last_kernel(NoiseArgs N) {
  if (threadIdx.x != 0) return;
  double t = 0.0;
  for (uint32_t b = 0; b < kNoiseGrid; ++b) t += N.part[b];
  N.part[kNoiseGrid] = sqrt(t / (double)N.npix);
}

}  // namespace

// Streaming kernels: at most 2048 workgroups, the rest by the grid stride.
hipError_t launch_accum_fold(const FoldArgs& a, hipStream_t s) {
  const uint32_t grid = min((a.npix + kFoldBlock - 1) / kFoldBlock, 2048u);
  hipLaunchKernelGGL(accum_fold_kernel, dim3(grid ? grid : 1), dim3(kFoldBlock), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_accum_resolve(const ResolveArgs& a, hipStream_t s) {
  const uint32_t grid = (uint32_t)min(((size_t)a.npix * 3 + 255) / 256, (size_t)2048);
  hipLaunchKernelGGL(accum_resolve_kernel, dim3(grid ? grid : 1), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_accum_noise(const NoiseArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(accum_noise_kernel, dim3(kNoiseGrid), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(accum_noise_last_kernel, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace rtwk

// ------------------------------------------------- host loop (the CLI's) ----
// rtw::renderProgressive (rtw_host.hpp): the pass loop a host drives through
// the C ABI — accumulator, one workspace sized for a pass, resolve after every
// pass — with the device buffers it needs.
#include <algorithm>

#include "rtw_host.hpp"

namespace rtw {

std::vector<uint8_t> renderProgressive(const rtw_camera& cam, const rtw_params& p, uint32_t pass_spp,
                                       const FlatScene* scene, const rtw_world_desc* world, double max_noise,
                                       const PassFn& on_pass, uint32_t* samples_used) {
  if ((scene != nullptr) == (world != nullptr)) throw Error(RTW_EINVAL, "renderProgressive: a scene or a world");
  struct Dev {  // released on every way out
    rtw_scene sc = nullptr;
    rtw_world w = nullptr;
    rtw_accum acc = nullptr;
    void *ws = nullptr, *rgb = nullptr;
    ~Dev() {
      if (ws) (void)hipFree(ws);
      if (rgb) (void)hipFree(rgb);
      rtw_accum_destroy(acc);
      rtw_scene_destroy(sc);
      rtw_world_destroy(w);
    }
  } d;
  auto ok = [](int st) {
    if (st != RTW_OK) throw Error(st, rtw_last_error());
  };
  if (scene)
    ok(rtw_scene_create(scene->spheres.data(), (uint32_t)scene->spheres.size(), scene->materials.data(),
                        (uint32_t)scene->materials.size(), &d.sc));
  else
    ok(rtw_world_create(world, 0, &d.w));
  ok(rtw_accum_create(&p, &d.acc));
  const uint32_t first = std::min(pass_spp, p.spp);  // (a shorter last pass fits the same workspace)
  const size_t wsb = scene ? rtw_accum_workspace_bytes(&p, first) : rtw_accum_world_workspace_bytes(d.w, &p, first);
  if (wsb == 0) throw Error(RTW_EINVAL, rtw_last_error());
  std::vector<uint8_t> rgb((size_t)p.width * p.row_count * 3);
  if (hipMalloc(&d.ws, wsb) != hipSuccess || hipMalloc(&d.rgb, rgb.size()) != hipSuccess)
    throw Error(RTW_ENOMEM, "renderProgressive: device allocation failed");
  uint32_t done = 0;
  for (uint32_t pass = 1; done < p.spp; ++pass) {
    const uint32_t n = std::min(pass_spp, p.spp - done);
    ok(scene ? rtw_accum_render_device(d.acc, d.sc, &cam, n, d.ws, wsb, nullptr, nullptr)
             : rtw_accum_world_render_device(d.acc, d.w, &cam, n, d.ws, wsb, nullptr, nullptr));
    ok(rtw_accum_resolve_device(d.acc, static_cast<uint8_t*>(d.rgb), nullptr, nullptr));
    if (hipMemcpy(rgb.data(), d.rgb, rgb.size(), hipMemcpyDeviceToHost) != hipSuccess)
      throw Error(RTW_EHIP, "renderProgressive: the pass failed on the device");
    ok(rtw_accum_samples(d.acc, &done));
    PassInfo info{pass, done, -1.0};
    if (rtw_accum_noise(d.acc, nullptr, &info.noise) != RTW_OK) info.noise = -1.0;  // (fewer than two full chunks)
    if (on_pass) on_pass(info, rgb);
    if (max_noise > 0.0 && info.noise >= 0.0 && info.noise <= max_noise) break;
  }
  if (samples_used) *samples_used = done;
  return rgb;
}

}  // namespace rtw
