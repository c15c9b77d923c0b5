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

#include "rtw_adaptive.hpp"
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

// ---------------------------------------------------- masked accumulator ----
//   accum_fold_kernel with a per-pixel predicate: the values of
// an active pixel take the same additions in the same order, its statistic
// the full chunks and its count the pass's samples; an inactive pixel's sum,
// stat and cnt are not written and its values of `partial` are not read (a
// masked pass never wrote them).  The same streaming shape: a wave's loads
// cover 512 contiguous bytes, lanes of inactive pixels switched off.
__global__ void __launch_bounds__(kFoldBlock) accum_fold_masked_kernel(MaskedFoldArgs M) {
  __shared__ double tile[2][kFoldTile];
  const FoldArgs& F = M.f;
  const uint32_t t = threadIdx.x;
  const size_t nflat = (size_t)F.npix * 3;
  const uint32_t n_tiles = (F.npix + kFoldBlock - 1) / kFoldBlock;
  double2* stat2 = reinterpret_cast<double2*>(F.stat);
  for (uint32_t ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
    const size_t base = (size_t)ti * kFoldTile + t;
    const uint32_t pix = ti * kFoldBlock + t;
    const bool pin = pix < F.npix && M.act[pix] != 0;
    bool in[3];
    double s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const size_t e = base + k * kFoldBlock;
      in[k] = e < nflat && M.act[e / 3] != 0;  // (value e belongs to pixel e / 3)
      s[k] = in[k] ? F.sum[e] : 0.0;
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
    if (pin) {
      if (F.n_full) stat2[pix] = y;
      M.cnt[pix] += M.pass_spp;
    }
    __syncthreads();  // the next tile's first chunk reuses tile[0]
  }
}

// The active set after a fold, a mask, a budget or a load.  One wave per 8x8
// tile, lane l = pixel l of the tile: an active pixel stays active unless the
// user's mask clears it or the criterion (rtw_adaptive.hpp) finds it
// converged; the wave's ballot is the tile's mask.  Padding lanes of edge
// tiles are never active.
__global__ void __launch_bounds__(256) accum_active_kernel(ActiveArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);  // (wave-uniform)
  if (tile >= A.n_tiles) return;
  const uint32_t ty = tile / A.tiles_x, tx = tile - ty * A.tiles_x;
  const uint32_t px = tx * kTileW + (lane & 7u), ly = ty * kTileH + (lane >> 3);
  bool on = false;
  if (px < A.W && ly < A.rows) {
    const uint32_t pix = ly * A.W + px;
    on = A.from_cnt ? A.cnt[pix] == A.done : A.act[pix] != 0;
    if (on && A.user) on = A.user[pix] != 0;
    if (on && A.thr > 0.0) {
      const double2 y = reinterpret_cast<const double2*>(A.stat)[pix];
      on = !rtwa::pixel_converged(y.x, y.y, A.cnt[pix], A.chunk, A.min_spp, A.thr);
    }
    A.act[pix] = on ? 1 : 0;
  }
  const uint64_t m = __ballot(on);
  if (lane == 0) A.tile_mask[tile] = m;
}

// Compacts the non-empty tiles into tile_list in ascending order and counts
// them and their pixels: one workgroup, thread t scans the contiguous tiles
// [t * per, (t + 1) * per), an exclusive scan over the threads' counts places
// them.  No atomics: the same masks always give the same list.
__global__ void __launch_bounds__(1024) accum_compact_kernel(ActiveArgs A) {
  __shared__ uint32_t scan[1024];
  __shared__ uint32_t pixs[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (A.n_tiles + 1023u) / 1024u;
  const uint32_t lo = min(t * per, A.n_tiles), hi = min(lo + per, A.n_tiles);
  uint32_t n = 0, np = 0;
  for (uint32_t i = lo; i < hi; ++i) {
    const uint64_t m = A.tile_mask[i];
    n += m != 0ull;
    np += (uint32_t)__popcll(m);
  }
  scan[t] = n;
  pixs[t] = np;
  __syncthreads();
  for (uint32_t d = 1; d < 1024u; d <<= 1) {  // inclusive scan (Hillis-Steele)
    const uint32_t a = t >= d ? scan[t - d] : 0u, b = t >= d ? pixs[t - d] : 0u;
    __syncthreads();
    scan[t] += a;
    pixs[t] += b;
    __syncthreads();
  }
  uint32_t pos = scan[t] - n;
  for (uint32_t i = lo; i < hi; ++i)
    if (A.tile_mask[i] != 0ull) A.tile_list[pos++] = i;
  if (t == 1023u) {
    A.n_active[0] = scan[t];
    A.n_active[1] = pixs[t];
  }
}

// accum_resolve_kernel with the pixel's own scale, 1 / cnt; a pixel without a
// sample resolves to 0.
__global__ void __launch_bounds__(256) accum_resolve_cnt_kernel(ResolveCntArgs F) {
  const size_t nflat = (size_t)F.npix * 3;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nflat; e += (size_t)gridDim.x * blockDim.x) {
    const uint32_t n = F.cnt[e / 3];
    if (n == 0u) {
      F.rgb[e] = 0;
      if (F.mean) F.mean[e] = 0.0f;
      continue;
    }
    const double scale = 1.0 / (double)n;
    const double t = F.sum[e];
    const double g = sqrt(t * scale);
    const double cl = fmax(0.0, fmin(g, 0.999));
    F.rgb[e] = (uint8_t)(256.0 * cl);
    if (F.mean) F.mean[e] = (float)(t * scale);
  }
}

// accum_noise_kernel with each pixel's own m = cnt / chunk; pixels with m < 2
// are left out of the sum and of the divisor.  The same fixed grid and trees.
__global__ void __launch_bounds__(256) accum_noise_cnt_kernel(NoiseCntArgs N) {
  __shared__ double red[256];
  __shared__ double redn[256];
  const double2* stat2 = reinterpret_cast<const double2*>(N.stat);
  double acc = 0.0, used = 0.0;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < N.npix; i += kNoiseGrid * 256u) {
    const uint32_t m = N.cnt[i] / N.chunk;
    if (m < 2u) continue;
    const double2 y = stat2[i];
    acc += rtwa::pixel_se2(y.x, y.y, m, N.chunk);
    used += 1.0;
  }
  red[threadIdx.x] = acc;
  redn[threadIdx.x] = used;
  __syncthreads();
  for (uint32_t w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      red[threadIdx.x] += red[threadIdx.x + w];
      redn[threadIdx.x] += redn[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    N.part[blockIdx.x] = red[0];
    N.part[kNoiseGrid + 1 + blockIdx.x] = redn[0];
  }
}
__global__ void __launch_bounds__(64) accum_noise_cnt_last_kernel(NoiseCntArgs N) {
  if (threadIdx.x != 0) return;
  double t = 0.0, n = 0.0;
  for (uint32_t b = 0; b < kNoiseGrid; ++b) t += N.part[b], n += N.part[kNoiseGrid + 1 + b];
  N.part[kNoiseGrid] = n > 0.0 ? sqrt(t / n) : 0.0;
  N.part[2 * kNoiseGrid + 1] = n;
}

__global__ void __launch_bounds__(256) accum_fill_u32_kernel(uint32_t* p, uint32_t n, uint32_t v) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) p[i] = v;
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

hipError_t launch_accum_fold_masked(const MaskedFoldArgs& a, hipStream_t s) {
  const uint32_t grid = min((a.f.npix + kFoldBlock - 1) / kFoldBlock, 2048u);
  hipLaunchKernelGGL(accum_fold_masked_kernel, dim3(grid ? grid : 1), dim3(kFoldBlock), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_accum_active(const ActiveArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(accum_active_kernel, dim3((a.n_tiles + 3) / 4), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(accum_compact_kernel, dim3(1), dim3(1024), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_accum_resolve_cnt(const ResolveCntArgs& a, hipStream_t s) {
  const uint32_t grid = (uint32_t)min(((size_t)a.npix * 3 + 255) / 256, (size_t)2048);
  hipLaunchKernelGGL(accum_resolve_cnt_kernel, dim3(grid ? grid : 1), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_accum_noise_cnt(const NoiseCntArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(accum_noise_cnt_kernel, dim3(kNoiseGrid), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(accum_noise_cnt_last_kernel, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_accum_fill_u32(uint32_t* p, uint32_t n, uint32_t v, hipStream_t s) {
  const uint32_t grid = min((n + 255u) / 256u, 2048u);
  hipLaunchKernelGGL(accum_fill_u32_kernel, dim3(grid ? grid : 1), dim3(256), 0, s, p, n, v);
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
                                       const PassFn& on_pass, uint32_t* samples_used, const AdaptiveOpts* adaptive,
                                       const rtw_denoise_opts* denoise) {
  if ((scene != nullptr) == (world != nullptr)) throw Error(RTW_EINVAL, "renderProgressive: a scene or a world");
  struct Dev {  // released on every way out
    rtw_scene sc = nullptr;
    rtw_world w = nullptr;
    rtw_accum acc = nullptr;
    void *ws = nullptr, *rgb = nullptr, *guides = nullptr, *dn_ws = nullptr;
    ~Dev() {
      if (ws) (void)hipFree(ws);
      if (rgb) (void)hipFree(rgb);
      if (guides) (void)hipFree(guides);
      if (dn_ws) (void)hipFree(dn_ws);
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
  const bool budget = adaptive && adaptive->pixel_noise > 0.0;
  if (budget) ok(rtw_accum_set_adaptive(d.acc, adaptive->pixel_noise, adaptive->min_spp));
  const uint32_t first = std::min(pass_spp, p.spp);  // (a shorter last pass fits the same workspace)
  const size_t wsb = scene ? rtw_accum_workspace_bytes(&p, first) : rtw_accum_world_workspace_bytes(d.w, &p, first);
  if (wsb == 0) throw Error(RTW_EINVAL, rtw_last_error());
  std::vector<uint8_t> rgb((size_t)p.width * p.row_count * 3);
  if (hipMalloc(&d.ws, wsb) != hipSuccess || hipMalloc(&d.rgb, rgb.size()) != hipSuccess)
    throw Error(RTW_ENOMEM, "renderProgressive: device allocation failed");
  size_t dn_bytes = 0;
  if (denoise) {  // the guides, once per run
    dn_bytes = rtw_accum_denoise_workspace_bytes(d.acc, denoise);
    if (dn_bytes == 0) throw Error(RTW_EINVAL, rtw_last_error());
    if (hipMalloc(&d.guides, (size_t)p.width * p.row_count * sizeof(rtw_guide)) != hipSuccess ||
        hipMalloc(&d.dn_ws, dn_bytes) != hipSuccess)
      throw Error(RTW_ENOMEM, "renderProgressive: device allocation failed");
    ok(scene ? rtw_scene_guides_device(d.sc, &cam, &p, static_cast<rtw_guide*>(d.guides), nullptr)
             : rtw_world_guides_device(d.w, &cam, &p, static_cast<rtw_guide*>(d.guides), nullptr));
  }
  uint32_t done = 0;
  for (uint32_t pass = 1; done < p.spp; ++pass) {
    if (budget) {  // every pixel within its budget: the frame is done
      uint32_t pixels = 0, tiles = 0;
      ok(rtw_accum_active(d.acc, &pixels, &tiles));
      if (pixels == 0) break;
    }
    const uint32_t n = std::min(pass_spp, p.spp - done);
    ok(scene ? rtw_accum_render_device(d.acc, d.sc, &cam, n, d.ws, wsb, nullptr, nullptr)
             : rtw_accum_world_render_device(d.acc, d.w, &cam, n, d.ws, wsb, nullptr, nullptr));
    if (denoise)
      ok(rtw_accum_denoise_device(d.acc, static_cast<const rtw_guide*>(d.guides), denoise, d.dn_ws, dn_bytes,
                                  static_cast<uint8_t*>(d.rgb), nullptr, nullptr));
    else
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
  if (adaptive && adaptive->counts) {
    adaptive->counts->resize((size_t)p.width * p.row_count);
    ok(rtw_accum_read_counts(d.acc, adaptive->counts->data()));
  }
  return rgb;
}

void writeCountsPGM(const std::string& path, const std::vector<uint32_t>& counts, uint32_t w, uint32_t h) {
  if (counts.size() != (size_t)w * h) throw Error(RTW_EINVAL, "writeCountsPGM: counts do not have the image's size");
  const uint32_t top = counts.empty() ? 0u : *std::max_element(counts.begin(), counts.end());
  if (top > 65535u) throw Error(RTW_UNSUPPORTED, "writeCountsPGM: a count above 65535");
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) throw Error(RTW_EINVAL, "cannot write " + path);
  const bool wide = top > 255u;
  std::fprintf(f, "P5\n%u %u\n%u\n", w, h, wide ? 65535u : 255u);
  std::vector<uint8_t> row;
  for (uint32_t c : counts) {
    if (wide) row.push_back((uint8_t)(c >> 8));
    row.push_back((uint8_t)(c & 255u));
  }
  std::fwrite(row.data(), 1, row.size(), f);
  std::fclose(f);
}

}  // namespace rtw
