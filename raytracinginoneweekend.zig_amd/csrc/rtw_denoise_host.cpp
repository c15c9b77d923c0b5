// rtw_denoise_host.cpp — the denoiser on the CPU (rtw_hip.h rtw_denoise_host):
// rtw_denoise.hpp's filter_pixel over host buffers, level by level, as the
// device kernels (rtw_denoise.hip) run it.  The restatement the device's bytes
// are compared with; no HIP here, so it runs on a machine without a GPU.
// Also the argument checks and workspace size both entries share, and the
// spatial variance estimate over host buffers (rtw_denoise_spatial_variance_host).
#include <cstring>

#include "rtw_denoise.hpp"
#include "rtw_hip.h"

int rtw_fail(int status, const char* fmt, ...);  // rtw_capi.hip: sets rtw_last_error

static_assert(sizeof(rtw_guide) == sizeof(rtwd::Guide) && alignof(rtwd::Guide) == 16, "rtw_guide is rtwd::Guide");
static_assert(RTW_DENOISE_MAX_LEVELS == rtwd::kMaxLevels && RTW_DENOISE_NO_COLOR == rtwd::kFlagNoColor, "rtw_hip.h");
static_assert(RTW_DENOISE_DIRECT == rtwd::kFlagDirect && RTW_DENOISE_SPATIAL_VAR == rtwd::kFlagSpatialVar, "rtw_hip.h");

namespace rtwd {

int check_call(const char* who, const void* mean, uint32_t W, uint32_t H, uint32_t levels, double sc, double sn,
               double sd, double sa, uint32_t flags, const void* workspace, size_t workspace_bytes, const void* rgb_out,
               const void* mean_out, Params& P) {
  if (!mean) return rtw_fail(RTW_EINVAL, "%s: the mean image is NULL", who);
  if (!rgb_out && !mean_out) return rtw_fail(RTW_EINVAL, "%s: rgb_out and mean_out are both NULL", who);
  if (W == 0 || H == 0 || W > 65536u || H > 65536u || (uint64_t)W * H > (1ull << 28))
    return rtw_fail(RTW_EINVAL, "%s: image of %u x %u pixels", who, W, H);
  if (!resolve(levels, sc, sn, sd, sa, flags, P))
    return rtw_fail(RTW_EINVAL, "%s: options out of range (levels %u of at most %u, a negative sigma or flags 0x%x)",
                    who, levels, kMaxLevels, flags);
  if (!workspace) return rtw_fail(RTW_EINVAL, "%s: workspace is NULL", who);
  if (((uintptr_t)workspace & 15u) != 0) return rtw_fail(RTW_EINVAL, "%s: workspace is not 16-byte aligned", who);
  const size_t need = 2 * image_bytes(W, H);
  if (workspace_bytes < need)
    return rtw_fail(RTW_EINVAL, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  return RTW_OK;
}

int check_spatial_call(const char* who, const void* mean, const void* var_in, const void* guides, uint32_t W, uint32_t H,
                       uint32_t levels, double sc, double sn, double sd, double sa, uint32_t flags, const void* var_out,
                       Params& P) {
  if (!mean) return rtw_fail(RTW_EINVAL, "%s: the mean image is NULL", who);
  if (!var_out) return rtw_fail(RTW_EINVAL, "%s: var_out is NULL", who);
  if (W == 0 || H == 0 || W > 65536u || H > 65536u || (uint64_t)W * H > (1ull << 28))
    return rtw_fail(RTW_EINVAL, "%s: image of %u x %u pixels", who, W, H);
  if (!resolve(levels, sc, sn, sd, sa, flags, P))
    return rtw_fail(RTW_EINVAL, "%s: options out of range (levels %u of at most %u, a negative sigma or flags 0x%x)",
                    who, levels, kMaxLevels, flags);
  if (var_out == mean || var_out == var_in || var_out == guides)
    return rtw_fail(RTW_EINVAL, "%s: var_out aliases an input", who);
  return RTW_OK;
}

void spatial_variance_image(const float* mean, const float* var_in, const Guide* G, uint32_t W, uint32_t H,
                            const Params& P, float* var_out) {
  const int w = (int)W, h = (int)H;
  auto tap = [&](int x, int y) {
    const size_t i = (size_t)y * W + x;
    return sv_tap(Px{mean[3 * i], mean[3 * i + 1], mean[3 * i + 2], var_in ? var_in[i] : kVarUnknown});
  };
  auto gd = [&](int x, int y) { return G[(size_t)y * W + x]; };
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t i = (size_t)y * W + x;
      const float vp = var_in ? var_in[i] : kVarUnknown;
      var_out[i] = G ? spatial_variance_pixel<true>(x, y, w, h, P, vp, tap, gd)
                     : spatial_variance_pixel<false>(x, y, w, h, P, vp, tap, gd);
    }
}

}  // namespace rtwd

extern "C" {

size_t rtw_denoise_workspace_bytes(uint32_t W, uint32_t H, const rtw_denoise_opts* o) {
  rtwd::Params P;
  if (W == 0 || H == 0 || W > 65536u || H > 65536u || (uint64_t)W * H > (1ull << 28)) {
    rtw_fail(RTW_EINVAL, "rtw_denoise_workspace_bytes: image of %u x %u pixels", W, H);
    return 0;
  }
  if (o && !rtwd::resolve(o->levels, o->sigma_color, o->sigma_normal, o->sigma_depth, o->sigma_albedo, o->flags, P)) {
    rtw_fail(RTW_EINVAL, "rtw_denoise_workspace_bytes: options out of range");
    return 0;
  }
  return 2 * rtwd::image_bytes(W, H);
}

int rtw_denoise_host(const float* mean, const float* var, const rtw_guide* guides, uint32_t W, uint32_t H,
                     const rtw_denoise_opts* o, void* workspace, size_t workspace_bytes, uint8_t* rgb_out,
                     float* mean_out, void* /*stream*/) {
  using namespace rtwd;
  const rtw_denoise_opts dflt{};
  if (!o) o = &dflt;
  Params P;
  const int st = check_call("rtw_denoise_host", mean, W, H, o->levels, o->sigma_color, o->sigma_normal, o->sigma_depth,
                            o->sigma_albedo, o->flags, workspace, workspace_bytes, rgb_out, mean_out, P);
  if (st != RTW_OK) return st;
  Px* buf[2] = {static_cast<Px*>(workspace),
                reinterpret_cast<Px*>(static_cast<unsigned char*>(workspace) + image_bytes(W, H))};
  const Guide* G = reinterpret_cast<const Guide*>(guides);
  const int w = (int)W, h = (int)H;
  auto gd = [&](int x, int y) { return G[(size_t)y * W + x]; };
  if (P.flags & kFlagSpatialVar) {  // the estimated map lives in the second image: level 1 only reads it
    float* est = reinterpret_cast<float*>(buf[1]);
    spatial_variance_image(mean, var, G, W, H, P, est);
    var = est;
  }
  for (uint32_t l = 0; l < P.levels; ++l) {
    const Px* in = l ? buf[(l - 1) & 1u] : nullptr;
    Px* out = buf[l & 1u];
    auto px = [&](int x, int y) {
      const size_t i = (size_t)y * W + x;
      if (in) return in[i];
      return Px{mean[3 * i], mean[3 * i + 1], mean[3 * i + 2], var ? var[i] : kVarUnknown};
    };
    const bool last = l + 1 == P.levels;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const Px r = G ? filter_pixel<true>(x, y, w, h, 1 << l, P, px, gd)
                       : filter_pixel<false>(x, y, w, h, 1 << l, P, px, gd);
        const size_t i = (size_t)y * W + x;
        if (!last) {
          out[i] = r;
          continue;
        }
        if (mean_out) mean_out[3 * i] = r.r, mean_out[3 * i + 1] = r.g, mean_out[3 * i + 2] = r.b;
        if (rgb_out) {
          rgb_out[3 * i] = quantise((double)r.r);
          rgb_out[3 * i + 1] = quantise((double)r.g);
          rgb_out[3 * i + 2] = quantise((double)r.b);
        }
      }
  }
  return RTW_OK;
}

int rtw_denoise_spatial_variance_host(const float* mean, const float* var_in, const rtw_guide* guides, uint32_t W,
                                      uint32_t H, const rtw_denoise_opts* o, float* var_out, void* /*stream*/) {
  const rtw_denoise_opts dflt{};
  if (!o) o = &dflt;
  rtwd::Params P;
  const int st = rtwd::check_spatial_call("rtw_denoise_spatial_variance_host", mean, var_in, guides, W, H, o->levels,
                                          o->sigma_color, o->sigma_normal, o->sigma_depth, o->sigma_albedo, o->flags,
                                          var_out, P);
  if (st != RTW_OK) return st;
  rtwd::spatial_variance_image(mean, var_in, reinterpret_cast<const rtwd::Guide*>(guides), W, H, P, var_out);
  return RTW_OK;
}

}  // extern "C"
