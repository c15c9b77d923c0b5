// rtw_temporal_clamp_host.cpp — the clamped temporal accumulation on the CPU
// (rtw_hip.h rtw_temporal_clamped_host): rtw_temporal_clamp.hpp's per-pixel
// function over host buffers, as the device kernel (rtw_temporal_clamp.hip) runs
// it.  The restatement the device's bytes are compared with; no HIP here.  Also
// the check of rtw_temporal_clamp both forms share.
#include <cstring>

#include "rtw_hip.h"
#include "rtw_temporal_clamp.hpp"

int rtw_fail(int status, const char* fmt, ...);  // rtw_capi.hip: sets rtw_last_error

static_assert(sizeof(rtw_temporal_clamp) == 16, "rtw_hip.h");
static_assert(RTW_ABI_VERSION == 4, "new symbols only");

namespace rtwt {

int check_clamp(const char* who, double gamma, uint32_t radius, uint32_t reserved, Clamp& K) {
  if (!resolve_clamp(gamma, radius, reserved, K))
    return rtw_fail(RTW_EINVAL, "%s: clamp out of range (gamma %g, radius %u of at most %u, reserved 0x%x)", who, gamma,
                    radius, kMaxClampRadius, reserved);
  return RTW_OK;
}

}  // namespace rtwt

extern "C" {

int rtw_temporal_clamped_host(const float* mean, const rtw_guide* guides, const double* prev_p,
                              const rtw_camera* cam_prev, const rtw_camera* cam, const rtw_history* hist_in, uint32_t W,
                              uint32_t H, const rtw_temporal_opts* o, const rtw_temporal_clamp* clamp,
                              rtw_history* hist_out, float* mean_out, float* var_out, void* stream) {
  using namespace rtwt;
  if (!clamp)
    return rtw_temporal_host(mean, guides, prev_p, cam_prev, cam, hist_in, W, H, o, hist_out, mean_out, var_out, stream);
  const char* who = "rtw_temporal_clamped_host";
  const rtw_temporal_opts dflt{};
  if (!o) o = &dflt;
  Params P;
  int st = check_call(who, mean, guides, prev_p, cam_prev, cam, hist_in, W, H, o->max_history, o->depth_tol,
                      o->min_len_var, o->flags, hist_out, mean_out, var_out, P);
  if (st != RTW_OK) return st;
  Clamp K;
  st = check_clamp(who, clamp->gamma, clamp->radius, clamp->reserved, K);
  if (st != RTW_OK) return st;
  const Proj proj = make_proj(cam_prev->origin, cam_prev->horizontal, cam_prev->vertical, cam_prev->lower_left_corner);
  const bool same_cam = std::memcmp(cam_prev, cam, sizeof(rtw_camera)) == 0;
  const Guide* G = reinterpret_cast<const Guide*>(guides);
  const History* HI = reinterpret_cast<const History*>(hist_in);
  History* HO = reinterpret_cast<History*>(hist_out);
  const int w = (int)W, h = (int)H;
  auto hist = [&](int x, int y) { return HI[(size_t)y * W + x]; };
  auto cur = [&](int x, int y) {
    if (x < 0 || x >= w || y < 0 || y >= h) return Rgb{NAN, NAN, NAN};
    const float* p = mean + 3 * ((size_t)y * W + x);
    return Rgb{p[0], p[1], p[2]};
  };
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t i = (size_t)y * W + x;
      const Out r = accumulate_pixel_clamped(x, y, w, h, P, K.gamma, K.radius, G[i], HI != nullptr, prev_p != nullptr,
                                             prev_p ? prev_p[3 * i] : 0.0, prev_p ? prev_p[3 * i + 1] : 0.0,
                                             prev_p ? prev_p[3 * i + 2] : 0.0, proj, same_cam, hist, cur);
      HO[i] = r.rec;
      if (mean_out) mean_out[3 * i] = r.rec.mean[0], mean_out[3 * i + 1] = r.rec.mean[1], mean_out[3 * i + 2] = r.rec.mean[2];
      if (var_out) var_out[i] = r.var;
    }
  return RTW_OK;
}

}  // extern "C"
