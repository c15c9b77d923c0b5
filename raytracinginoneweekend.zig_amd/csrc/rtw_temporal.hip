// rtw_temporal.hip — device side of temporal accumulation (rtw_hip.h
// rtw_temporal_device, rtw_pixel_rays_device, rtw_world_prev_points_device;
// DESIGN.md §18).  The arithmetic is rtw_temporal.hpp's, the functions
// rtw_temporal_host and rtw_world_prev_points_host run: the kernels here only
// decide where a record comes from, so the device's bytes are the host's.
//
// temporal_kernel: a workgroup is a tile of 64 x 4 pixels, a wave one row of 64
// consecutive x (denoise_level_kernel's shape): the centre's mean, guide, point
// and the three stores are coalesced.  Every record is read as whole 16-byte
// loads (history two, guide two).  The four taps are per-lane gathers from
// global memory: where nothing moved they are the lane's own record, where the
// scene moved neighbouring lanes read neighbouring records, and the history
// image (32 B per pixel) stays in L2 / the Infinity Cache.  No LDS, no atomics.
// prev_points_kernel and pixel_rays_kernel: one lane per record.
// -ffp-contract=off (Makefile).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "rtw_capi_shared.hpp"
#include "rtw_temporal.hpp"

namespace rtwk {

namespace {

using rtwt::Guide;
using rtwt::History;

constexpr int kTpTileW = 64, kTpTileH = 4;  // a wave = one row of the tile
constexpr int kTpBlock = kTpTileW * kTpTileH;

struct TemporalArgs {
  const float* mean;
  const Guide* guides;
  const double* prev_p;    // optional
  const History* hist_in;  // optional: null = the first frame
  History* hist_out;
  float* mean_out;  // optional
  float* var_out;   // optional
  int W, H;
  uint32_t same_cam;
  rtwt::Params P;
  rtwt::Proj proj;
};

__global__ void __launch_bounds__(kTpBlock) temporal_kernel(TemporalArgs A) {
  const int x = (int)blockIdx.x * kTpTileW + (int)(threadIdx.x & (kTpTileW - 1));
  const int y = (int)blockIdx.y * kTpTileH + (int)(threadIdx.x >> 6);
  if (x >= A.W || y >= A.H) return;
  const size_t i = (size_t)y * A.W + x;
  const float m0 = A.mean[3 * i], m1 = A.mean[3 * i + 1], m2 = A.mean[3 * i + 2];
  const Guide g = A.guides[i];
  double p0 = 0.0, p1 = 0.0, p2 = 0.0;
  if (A.prev_p) p0 = A.prev_p[3 * i], p1 = A.prev_p[3 * i + 1], p2 = A.prev_p[3 * i + 2];  // (uniform)
  auto hist = [&](int qx, int qy) { return A.hist_in[(size_t)qy * A.W + qx]; };
  const rtwt::Out r = rtwt::accumulate_pixel(x, y, A.W, A.H, A.P, m0, m1, m2, g, A.hist_in != nullptr,
                                             A.prev_p != nullptr, p0, p1, p2, A.proj, A.same_cam != 0u, hist);
  A.hist_out[i] = r.rec;
  if (A.mean_out) A.mean_out[3 * i] = r.rec.mean[0], A.mean_out[3 * i + 1] = r.rec.mean[1], A.mean_out[3 * i + 2] = r.rec.mean[2];
  if (A.var_out) A.var_out[i] = r.var;
}

struct PixelRaysArgs {
  double origin[3], horizontal[3], vertical[3], llc[3];
  double time0, time1;
  uint32_t W, H;
  double* rays;  // [H][W] rtw_ray (9 f64)
};

__global__ void __launch_bounds__(256) pixel_rays_kernel(PixelRaysArgs A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;  // (W * H <= 2^31)
  if (i >= A.W * A.H) return;
  const uint32_t y = i / A.W, x = i - y * A.W;
  double r[9];
  rtwt::pixel_ray(A.origin, A.horizontal, A.vertical, A.llc, A.time0, A.time1, A.W, A.H, x, y, r);
  double* o = A.rays + (size_t)9 * i;
#pragma unroll
  for (int k = 0; k < 9; ++k) o[k] = r[k];
}

struct PrevPointsArgs {
  const double* prim;     // the world's tables (WorldView's)
  const double* xform;
  const uint32_t* order;  // list index -> stored position
  uint32_t n_prims;
  uint32_t n;             // <= 2^31
  const double* hits;     // n x rtw_hit (10 x 8 bytes)
  const double* a_prev;   // n_prims x 9, list order, or null
  const double* xv_prev;  // n_xforms x kMaxXfOps x 3, or null
  double* out;            // n x 3
  double time;
};

__global__ void __launch_bounds__(256) prev_points_kernel(PrevPointsArgs A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= A.n) return;
  const double* h = A.hits + (size_t)10 * i;
  double* out = A.out + (size_t)3 * i;
  const uint64_t pf = reinterpret_cast<const uint64_t*>(h)[9];
  const uint32_t prim = (uint32_t)pf, front = (uint32_t)(pf >> 32);
  if (prim == 0u || prim > A.n_prims) {
    out[0] = 0.0, out[1] = 0.0, out[2] = 0.0;
    return;
  }
  const double p[3] = {h[1], h[2], h[3]}, nrm[3] = {h[4], h[5], h[6]};
  const bool moved = A.a_prev || A.xv_prev;  // (uniform)
  const double* rec = A.prim + (size_t)kWorldRec * A.order[prim - 1u];
  const uint32_t meta0 = rtwr::ld_u32(rec + 14, 0);
  const uint32_t kind = meta0 & 0xFFu, xf = meta0 >> 8;  // xf: transform index + 1
  double r[11];
  if (A.a_prev) {
    rtwr::fill_record(kind, A.a_prev + (size_t)9 * (prim - 1u), r);
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = rec[k];
  }
  uint32_t xf_h = 0u;
  const double *v_now = rec, *v_prev = rec;  // (not read without a chain)
  if (xf) {
    const double* x = A.xform + (size_t)kWorldRec * (xf - 1u);
    xf_h = rtwr::ld_u32(x, 0);
    v_now = x + 4;
    v_prev = A.xv_prev ? A.xv_prev + (size_t)3 * kMaxXfOps * (xf - 1u) : v_now;
  }
  double q[3];
  rtwt::prev_point(p, nrm, h[7], h[8], front, kind, r, xf_h, v_now, v_prev, A.time, moved, q);
  out[0] = q[0], out[1] = q[1], out[2] = q[2];
}

}  // namespace

}  // namespace rtwk

extern "C" {

int rtw_temporal_device(const float* d_mean, const rtw_guide* d_guides, const double* d_prev_p,
                        const rtw_camera* cam_prev, const rtw_camera* cam, const rtw_history* d_hist_in, uint32_t W,
                        uint32_t H, const rtw_temporal_opts* o, rtw_history* d_hist_out, float* d_mean_out,
                        float* d_var_out, void* stream) {
  using namespace rtwk;
  const rtw_temporal_opts dflt{};
  if (!o) o = &dflt;
  TemporalArgs a;
  std::memset(&a, 0, sizeof(a));
  const int st = rtwt::check_call("rtw_temporal_device", d_mean, d_guides, d_prev_p, cam_prev, cam, d_hist_in, W, H,
                                  o->max_history, o->depth_tol, o->min_len_var, o->flags, d_hist_out, d_mean_out,
                                  d_var_out, a.P);
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
  a.proj = rtwt::make_proj(cam_prev->origin, cam_prev->horizontal, cam_prev->vertical, cam_prev->lower_left_corner);
  const dim3 grid((W + kTpTileW - 1) / kTpTileW, (H + kTpTileH - 1) / kTpTileH), block(kTpBlock);
  hipLaunchKernelGGL(temporal_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "rtw_temporal_device: kernel launch: %s", hipGetErrorString(e));
  return RTW_OK;
}

int rtw_pixel_rays_device(const rtw_camera* cam, uint32_t W, uint32_t H, rtw_ray* d_rays, void* stream) {
  using namespace rtwk;
  if (!cam || !d_rays) return rtw_fail(RTW_EINVAL, "rtw_pixel_rays_device: cam or d_rays is NULL");
  if (W < 2 || H < 2 || (uint64_t)W * H > RTW_QUERY_MAX_RAYS)
    return rtw_fail(RTW_EINVAL, "rtw_pixel_rays_device: image of %u x %u pixels", W, H);
  if (((uintptr_t)d_rays & 7u) != 0) return rtw_fail(RTW_EINVAL, "rtw_pixel_rays_device: d_rays is not 8-byte aligned");
  PixelRaysArgs a;
  for (int k = 0; k < 3; ++k) {
    a.origin[k] = cam->origin[k], a.horizontal[k] = cam->horizontal[k], a.vertical[k] = cam->vertical[k];
    a.llc[k] = cam->lower_left_corner[k];
  }
  a.time0 = cam->time0, a.time1 = cam->time1;
  a.W = W, a.H = H;
  a.rays = reinterpret_cast<double*>(d_rays);
  const uint32_t n = W * H;  // (<= 2^31)
  hipLaunchKernelGGL(pixel_rays_kernel, dim3((n + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "rtw_pixel_rays_device: kernel launch: %s", hipGetErrorString(e));
  return RTW_OK;
}

int rtw_world_prev_points_device(rtw_world w, const rtw_hit* d_hits, uint64_t n, double time, const double* d_a_prev,
                                 const double* d_xv_prev, double* d_prev_p, void* stream) {
  using namespace rtwk;
  const char* who = "rtw_world_prev_points_device";
  WorldView view;
  uint32_t feat = 0;
  const int st = rtw_world_view(w, who, &view, &feat);  // (the world's device must be current)
  if (st != RTW_OK) return st;
  if (feat & 64u)  // rtw_world_walk.hpp kFeatTri
    return rtw_fail(RTW_UNSUPPORTED, "%s: the world holds triangles: previous points are not built for them", who);
  if (n > RTW_QUERY_MAX_RAYS || !std::isfinite(time)) return rtw_fail(RTW_EINVAL, "%s: n > 2^31 or a non-finite time", who);
  if (n == 0) return RTW_OK;
  if (!d_hits || !d_prev_p) return rtw_fail(RTW_EINVAL, "%s: d_hits or d_prev_p is NULL", who);
  if ((((uintptr_t)d_hits | (uintptr_t)d_prev_p | (uintptr_t)d_a_prev | (uintptr_t)d_xv_prev) & 7u) != 0)
    return rtw_fail(RTW_EINVAL, "%s: a buffer is not 8-byte aligned", who);
  PrevPointsArgs a;
  a.prim = view.prim, a.xform = view.xform, a.order = view.order, a.n_prims = view.n_prims;
  a.n = (uint32_t)n;
  a.hits = reinterpret_cast<const double*>(d_hits);
  a.a_prev = d_a_prev, a.xv_prev = d_xv_prev;
  a.out = d_prev_p;
  a.time = time;
  hipLaunchKernelGGL(prev_points_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "%s: kernel launch: %s", who, hipGetErrorString(e));
  return RTW_OK;
}

}  // extern "C"
