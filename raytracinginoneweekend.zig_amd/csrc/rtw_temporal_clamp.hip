// rtw_temporal_clamp.hip — device side of the clamped temporal accumulation
// (rtw_hip.h rtw_temporal_clamped_device).  The arithmetic is
// rtw_temporal_clamp.hpp's, the function rtw_temporal_clamped_host runs: the
// kernel only decides where a value comes from, so the device's bytes are the
// host's.
//
// temporal_clamp_kernel: temporal_kernel's shape, a workgroup is a tile of
// 64 x 4 pixels and a wave one row of 64 consecutive x, so the guide, the point
// and the three stores stay coalesced and the history taps stay per-lane global
// gathers.  The current mean of the tile plus its halo of r pixels is staged in
// LDS, (64 + 2r) x (4 + 2r) pixels of three floats, interleaved as in memory:
// a staged row is one contiguous run of 3 (64 + 2r) floats of the image, which a
// wave copies with consecutive lanes on consecutive floats (coalesced loads,
// consecutive LDS dwords).  A window read has lane l at dword 3 l + const: 3 is
// odd, so the 32 lanes of a half-wave fall on 32 different banks.  A halo pixel
// outside the image is staged as NaN and skipped by the arithmetic's finite
// rule.  Every lane takes part in the staging and reaches the barrier; lanes
// outside the image drop out after it.  No atomics.  -ffp-contract=off (Makefile).
#include <hip/hip_runtime.h>

#include <cstring>

#include "rtw_capi_shared.hpp"
#include "rtw_temporal_clamp.hpp"

namespace rtwk {

namespace {

using rtwt::Guide;
using rtwt::History;

constexpr int kTcTileW = 64, kTcTileH = 4;  // a wave = one row of the tile
constexpr int kTcBlock = kTcTileW * kTcTileH;
constexpr int kTcMaxR = (int)rtwt::kMaxClampRadius;
constexpr int kTcLdsFloats = 3 * (kTcTileW + 2 * kTcMaxR) * (kTcTileH + 2 * kTcMaxR);  // 2100 floats, 8400 bytes

struct TemporalClampArgs {
  const float* mean;
  const Guide* guides;
  const double* prev_p;    // optional
  const History* hist_in;  // optional: null = the first frame
  History* hist_out;
  float* mean_out;  // optional
  float* var_out;   // optional
  int W, H;
  uint32_t same_cam;
  int radius;  // 1..kTcMaxR
  double gamma;
  rtwt::Params P;
  rtwt::Proj proj;
};

__global__ void __launch_bounds__(kTcBlock) temporal_clamp_kernel(TemporalClampArgs A) {
  __shared__ float tile[kTcLdsFloats];
  const int lane = (int)(threadIdx.x & (kTcTileW - 1)), wave = (int)(threadIdx.x >> 6);
  const int r = A.radius;
  const int tx0 = (int)blockIdx.x * kTcTileW - r, ty0 = (int)blockIdx.y * kTcTileH - r;  // the staged region's corner
  const int tw = kTcTileW + 2 * r, th = kTcTileH + 2 * r, rowf = 3 * tw;
  for (int ry = wave; ry < th; ry += kTcTileH) {  // (th <= 10, rowf <= 210: inside tile[])
    const int gy = ty0 + ry;
    const bool row_in = gy >= 0 && gy < A.H;
    const ptrdiff_t row = ((ptrdiff_t)gy * A.W + tx0) * 3;
    for (int k = lane; k < rowf; k += kTcTileW) {
      const int gx = tx0 + k / 3;
      float v = __builtin_nanf("");
      if (row_in && gx >= 0 && gx < A.W) v = A.mean[row + k];
      tile[ry * rowf + k] = v;
    }
  }
  __syncthreads();
  const int x = (int)blockIdx.x * kTcTileW + lane;
  const int y = (int)blockIdx.y * kTcTileH + wave;
  if (x >= A.W || y >= A.H) return;
  const size_t i = (size_t)y * A.W + x;
  const Guide g = A.guides[i];
  double p0 = 0.0, p1 = 0.0, p2 = 0.0;
  if (A.prev_p) p0 = A.prev_p[3 * i], p1 = A.prev_p[3 * i + 1], p2 = A.prev_p[3 * i + 2];  // (uniform)
  auto hist = [&](int qx, int qy) { return A.hist_in[(size_t)qy * A.W + qx]; };
  auto cur = [&](int qx, int qy) {  // (|qx - x|, |qy - y| <= r: inside the staged region)
    const float* p = tile + ((qy - ty0) * tw + (qx - tx0)) * 3;
    return rtwt::Rgb{p[0], p[1], p[2]};
  };
  const rtwt::Out o = rtwt::accumulate_pixel_clamped(x, y, A.W, A.H, A.P, A.gamma, r, g, A.hist_in != nullptr,
                                                     A.prev_p != nullptr, p0, p1, p2, A.proj, A.same_cam != 0u, hist, cur);
  A.hist_out[i] = o.rec;
  if (A.mean_out) A.mean_out[3 * i] = o.rec.mean[0], A.mean_out[3 * i + 1] = o.rec.mean[1], A.mean_out[3 * i + 2] = o.rec.mean[2];
  if (A.var_out) A.var_out[i] = o.var;
}

}  // namespace

}  // namespace rtwk

extern "C" {

int rtw_temporal_clamped_device(const float* d_mean, const rtw_guide* d_guides, const double* d_prev_p,
                                const rtw_camera* cam_prev, const rtw_camera* cam, const rtw_history* d_hist_in,
                                uint32_t W, uint32_t H, const rtw_temporal_opts* o, const rtw_temporal_clamp* clamp,
                                rtw_history* d_hist_out, float* d_mean_out, float* d_var_out, void* stream) {
  using namespace rtwk;
  if (!clamp)
    return rtw_temporal_device(d_mean, d_guides, d_prev_p, cam_prev, cam, d_hist_in, W, H, o, d_hist_out, d_mean_out,
                               d_var_out, stream);
  const char* who = "rtw_temporal_clamped_device";
  const rtw_temporal_opts dflt{};
  if (!o) o = &dflt;
  TemporalClampArgs a;
  std::memset(&a, 0, sizeof(a));
  int st = rtwt::check_call(who, d_mean, d_guides, d_prev_p, cam_prev, cam, d_hist_in, W, H, o->max_history, o->depth_tol,
                            o->min_len_var, o->flags, d_hist_out, d_mean_out, d_var_out, a.P);
  if (st != RTW_OK) return st;
  rtwt::Clamp K;
  st = rtwt::check_clamp(who, clamp->gamma, clamp->radius, clamp->reserved, K);
  if (st != RTW_OK) return st;
  a.mean = d_mean;
  a.guides = reinterpret_cast<const Guide*>(d_guides);
  a.prev_p = d_prev_p;
  a.hist_in = reinterpret_cast<const History*>(d_hist_in);
  a.hist_out = reinterpret_cast<History*>(d_hist_out);
  a.mean_out = d_mean_out;
  a.var_out = d_var_out;
  a.W = (int)W, a.H = (int)H;
  a.same_cam = std::memcmp(cam_prev, cam, sizeof(rtw_camera)) == 0 ? 1u : 0u;
  a.radius = K.radius, a.gamma = K.gamma;
  a.proj = rtwt::make_proj(cam_prev->origin, cam_prev->horizontal, cam_prev->vertical, cam_prev->lower_left_corner);
  const dim3 grid((W + kTcTileW - 1) / kTcTileW, (H + kTcTileH - 1) / kTcTileH), block(kTcBlock);
  hipLaunchKernelGGL(temporal_clamp_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "%s: kernel launch: %s", who, hipGetErrorString(e));
  return RTW_OK;
}

}  // extern "C"
