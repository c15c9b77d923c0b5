// rtw_temporal_host.cpp — temporal accumulation on the CPU (rtw_hip.h
// rtw_temporal_host, rtw_world_prev_points_host): rtw_temporal.hpp's per-pixel
// and per-hit functions over host buffers, as the device kernels
// (rtw_temporal.hip) run them.  The restatement the device's bytes are compared
// with; no HIP here, so it runs on a machine without a GPU.  Also the argument
// check both forms of rtw_temporal_* share.
#include <cstring>

#include "rtw_hip.h"
#include "rtw_temporal.hpp"

int rtw_fail(int status, const char* fmt, ...);  // rtw_capi.hip: sets rtw_last_error

static_assert(sizeof(rtw_history) == sizeof(rtwt::History) && alignof(rtwt::History) == 16, "rtw_history is rtwt::History");
static_assert(sizeof(rtw_hit) == 80 && sizeof(rtw_ray) == 72, "rtw_hip.h");
static_assert(RTW_MAX_XFORM_OPS == rtwk::kMaxXfOps, "rtw_hip.h");

namespace rtwt {

int check_call(const char* who, const void* mean, const void* guides, const void* prev_p, const void* cam_prev,
               const void* cam, const void* hist_in, uint32_t W, uint32_t H, uint32_t max_history, double depth_tol,
               uint32_t min_len_var, uint32_t flags, const void* hist_out, const void* mean_out, const void* var_out,
               Params& P) {
  if (!mean || !guides || !cam_prev || !cam || !hist_out)
    return rtw_fail(RTW_EINVAL, "%s: mean, guides, cam_prev, cam or hist_out is NULL", who);
  if (W < 2 || H < 2 || W > 65536u || H > 65536u || (uint64_t)W * H > (1ull << 28))
    return rtw_fail(RTW_EINVAL, "%s: image of %u x %u pixels", who, W, H);
  if (!resolve(max_history, depth_tol, min_len_var, flags, P))
    return rtw_fail(RTW_EINVAL,
                    "%s: options out of range (max_history %u of at most %u, depth_tol %g, min_len_var %u, flags 0x%x)",
                    who, max_history, kMaxMaxHistory, depth_tol, min_len_var, flags);
  if ((((uintptr_t)guides | (uintptr_t)hist_in | (uintptr_t)hist_out) & 15u) != 0)
    return rtw_fail(RTW_EINVAL, "%s: guides or a history image is not 16-byte aligned", who);
  if (((uintptr_t)prev_p & 7u) != 0) return rtw_fail(RTW_EINVAL, "%s: prev_p is not 8-byte aligned", who);
  if ((((uintptr_t)mean | (uintptr_t)mean_out | (uintptr_t)var_out) & 3u) != 0)
    return rtw_fail(RTW_EINVAL, "%s: a float image is not 4-byte aligned", who);
  // No output may overlap an input or another output: byte ranges from the image's size (at most 2^28 pixels of
  // at most 32 bytes, so nothing here wraps), NULL buffers left out.
  struct Range {
    uintptr_t at;
    size_t bytes;
  };
  const size_t n = (size_t)W * H;
  const Range out[3] = {{(uintptr_t)hist_out, n * 32}, {(uintptr_t)mean_out, n * 12}, {(uintptr_t)var_out, n * 4}};
  const Range in[4] = {{(uintptr_t)mean, n * 12}, {(uintptr_t)guides, n * 32}, {(uintptr_t)prev_p, n * 24}, {(uintptr_t)hist_in, n * 32}};
  auto overlap = [](const Range& a, const Range& b) { return a.at && b.at && a.at < b.at + b.bytes && b.at < a.at + a.bytes; };
  for (int o = 0; o < 3; ++o) {
    for (const Range& i : in)
      if (overlap(out[o], i)) return rtw_fail(RTW_EINVAL, "%s: an output overlaps an input", who);
    for (int o2 = o + 1; o2 < 3; ++o2)
      if (overlap(out[o], out[o2])) return rtw_fail(RTW_EINVAL, "%s: two outputs overlap", who);
  }
  return RTW_OK;
}

}  // namespace rtwt

extern "C" {

int rtw_temporal_host(const float* mean, const rtw_guide* guides, const double* prev_p, const rtw_camera* cam_prev,
                      const rtw_camera* cam, const rtw_history* hist_in, uint32_t W, uint32_t H,
                      const rtw_temporal_opts* o, rtw_history* hist_out, float* mean_out, float* var_out,
                      void* /*stream*/) {
  using namespace rtwt;
  const rtw_temporal_opts dflt{};
  if (!o) o = &dflt;
  Params P;
  const int st = check_call("rtw_temporal_host", mean, guides, prev_p, cam_prev, cam, hist_in, W, H, o->max_history,
                            o->depth_tol, o->min_len_var, o->flags, hist_out, mean_out, var_out, P);
  if (st != RTW_OK) return st;
  const Proj proj = make_proj(cam_prev->origin, cam_prev->horizontal, cam_prev->vertical, cam_prev->lower_left_corner);
  const bool same_cam = std::memcmp(cam_prev, cam, sizeof(rtw_camera)) == 0;
  const Guide* G = reinterpret_cast<const Guide*>(guides);
  const History* HI = reinterpret_cast<const History*>(hist_in);
  History* HO = reinterpret_cast<History*>(hist_out);
  auto hist = [&](int x, int y) { return HI[(size_t)y * W + x]; };
  for (int y = 0; y < (int)H; ++y)
    for (int x = 0; x < (int)W; ++x) {
      const size_t i = (size_t)y * W + x;
      const Out r = accumulate_pixel(x, y, (int)W, (int)H, P, mean[3 * i], mean[3 * i + 1], mean[3 * i + 2], G[i],
                                     HI != nullptr, prev_p != nullptr, prev_p ? prev_p[3 * i] : 0.0,
                                     prev_p ? prev_p[3 * i + 1] : 0.0, prev_p ? prev_p[3 * i + 2] : 0.0, proj, same_cam, hist);
      HO[i] = r.rec;
      if (mean_out) mean_out[3 * i] = r.rec.mean[0], mean_out[3 * i + 1] = r.rec.mean[1], mean_out[3 * i + 2] = r.rec.mean[2];
      if (var_out) var_out[i] = r.var;
    }
  return RTW_OK;
}

int rtw_world_prev_points_host(const rtw_world_desc* d, const rtw_hit* hits, uint64_t n, double time,
                               const double* a_prev, const double* xv_prev, double* prev_p) {
  const char* who = "rtw_world_prev_points_host";
  if (!d || (n && (!hits || !prev_p))) return rtw_fail(RTW_EINVAL, "%s: desc, hits or prev_p is NULL", who);
  if ((d->n_prims && !d->prims) || (d->n_xforms && !d->xforms))
    return rtw_fail(RTW_EINVAL, "%s: NULL array with a non-zero count", who);
  if (n > RTW_QUERY_MAX_RAYS || !rtwt::finite(time)) return rtw_fail(RTW_EINVAL, "%s: n > 2^31 or a non-finite time", who);
  if ((((uintptr_t)hits | (uintptr_t)prev_p | (uintptr_t)a_prev | (uintptr_t)xv_prev) & 7u) != 0)
    return rtw_fail(RTW_EINVAL, "%s: a buffer is not 8-byte aligned", who);
  for (uint32_t i = 0; i < d->n_prims; ++i)
    if (d->prims[i].kind == RTW_PRIM_TRIANGLE)
      return rtw_fail(RTW_UNSUPPORTED, "%s: primitive %u is a triangle: previous points are not built for triangles", who, i);
  for (uint32_t i = 0; i < d->n_prims; ++i)
    if (d->prims[i].kind > RTW_PRIM_YZ_RECT || d->prims[i].xform < -1 || d->prims[i].xform >= (int32_t)d->n_xforms)
      return rtw_fail(RTW_EINVAL, "%s: primitive %u: kind %u, transform %d", who, i, d->prims[i].kind, d->prims[i].xform);
  for (uint32_t i = 0; i < d->n_xforms; ++i)
    if (d->xforms[i].n > RTW_MAX_XFORM_OPS) return rtw_fail(RTW_EINVAL, "%s: transform %u has %u ops", who, i, d->xforms[i].n);
  const bool moved = a_prev || xv_prev;
  for (uint64_t i = 0; i < n; ++i) {
    const rtw_hit& h = hits[i];
    double* out = prev_p + 3 * i;
    if (h.prim == 0u || h.prim > d->n_prims) {
      out[0] = out[1] = out[2] = 0.0;
      continue;
    }
    const rtw_prim& p = d->prims[h.prim - 1u];
    double r[11];
    rtwr::fill_record(p.kind, a_prev ? a_prev + (size_t)9 * (h.prim - 1u) : p.a, r);
    uint32_t xf_h = 0u;
    const double *v_now = nullptr, *v_prev = nullptr;
    if (p.xform >= 0) {
      const rtw_xform& x = d->xforms[p.xform];
      xf_h = x.n;
      for (uint32_t k = 0; k < x.n; ++k) xf_h |= (x.op[k] & 0xFu) << (8 + 4 * k);
      v_now = &x.v[0][0];
      v_prev = xv_prev ? xv_prev + (size_t)3 * RTW_MAX_XFORM_OPS * (size_t)p.xform : v_now;
    }
    rtwt::prev_point(h.p, h.normal, h.u, h.v, h.front, p.kind, r, xf_h, v_now, v_prev, time, moved, out);
  }
  return RTW_OK;
}

}  // extern "C"
