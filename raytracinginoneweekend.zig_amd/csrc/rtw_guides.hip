// rtw_guides.hip — the scene's feature buffers (rtw_hip.h
// rtw_scene_guides_device): the first hit of each pixel's
// feature ray over the packed sphere table, in f64.  One lane per pixel, a
// wave-uniform loop over the table (scalar record loads; scene_closest,
// rtw_scene_hit.hpp, shared with the scene's ray queries); the winner is the
// reference's — minimal effective root, ties to the later sphere of the list,
// the sequential loop after a NaN root — and its hit record
// and checker value are computed as the megakernel computes them
// (rtw_device.hpp scatter_hit).  Runs once per frame.
#include <hip/hip_runtime.h>

#include "rtw_capi_shared.hpp"
#include "rtw_guides.hpp"
#include "rtw_math.hpp"
#include "rtw_scene_hit.hpp"

namespace rtwk {

namespace {

using D = double;
using V = V3<D>;

__global__ void __launch_bounds__(kGuideTileW* kGuideTileH) scene_guides_kernel(SceneGuideArgs A) {
  uint32_t x, q;
  if (!guide_pixel(A.r, x, q)) return;
  const SceneView<D>& S = A.sc;
  V o, d;
  guide_ray(A.r, x, q, o, d);
  const D time = A.r.time, tmin = 0.001;
  const SceneHit sh = scene_closest<false>(S, o, d, time, tmin, (D)__builtin_huge_val());
  const int hit = sh.pos, hit_orig = sh.orig;
  const D hit_t = sh.t;
  if (hit < 0) {
    guide_store(A.r, x, q, mk(0.0, 0.0, 0.0), 0.0, ld3(A.r.bg), 0u);
    return;
  }
  const uint32_t meta = S.meta[hit];
  const V p = add(o, mul(d, hit_t));
  const V c = scene_center(S, (uint32_t)hit, meta, time);
  const V outward = divs(sub(p, c), S.rad[hit]);
  const V normal = dot(outward, d) < 0.0 ? outward : mul(outward, -1.0);
  const uint32_t mi = (meta >> 8) & 0xFFFu;
  const D* mp = S.mat + 8 * mi;
  const uint32_t kind = S.kind[mi];
  V albedo = ld3(mp);  // solid colour, checker even colour, metal albedo
  if (kind == 1u && rtwm::checker_odd(10.0 * p.x, 10.0 * p.y, 10.0 * p.z)) albedo = ld3(mp + 3);
  if (kind == 3u) albedo = mk(1.0, 1.0, 1.0);
  guide_store(A.r, x, q, normal, hit_t, albedo, (uint32_t)hit_orig + 1u);
}

}  // namespace

hipError_t launch_scene_guides(const SceneGuideArgs& a, hipStream_t s) {
  const dim3 grid((a.r.W + kGuideTileW - 1) / kGuideTileW, (a.r.row_count + kGuideTileH - 1) / kGuideTileH);
  hipLaunchKernelGGL(scene_guides_kernel, grid, dim3(kGuideTileW * kGuideTileH), 0, s, a);
  return hipGetLastError();
}

}  // namespace rtwk

// The feature ray's fields from the camera and the frame's geometry; the
// argument check of both guide entries.
int rtw_guide_ray_fill(rtwk::GuideRay& g, const char* who, const rtw_camera* cam, const rtw_params* p, void* d_guides) {
  if (!cam || !p || !d_guides) return rtw_fail(RTW_EINVAL, "%s: camera/params/d_guides is NULL", who);
  if (((uintptr_t)d_guides & 15u) != 0) return rtw_fail(RTW_EINVAL, "%s: d_guides is not 16-byte aligned", who);
  if (p->width < 2 || p->height < 2 || (uint64_t)p->width * p->height > (1ull << 28))
    return rtw_fail(RTW_EINVAL, "%s: image %ux%u", who, p->width, p->height);
  if (p->row_stride == 0 || p->row_count == 0 ||
      (uint64_t)p->row_begin + (uint64_t)(p->row_count - 1) * p->row_stride >= p->height)
    return rtw_fail(RTW_EINVAL, "%s: rows %u + k*%u (k < %u) exceed height %u", who, p->row_begin, p->row_stride,
                    p->row_count, p->height);
  for (int k = 0; k < 3; ++k) {
    g.origin[k] = cam->origin[k];
    g.horizontal[k] = cam->horizontal[k];
    g.vertical[k] = cam->vertical[k];
    g.llc[k] = cam->lower_left_corner[k];
    g.bg[k] = p->background[k];
  }
  g.time = cam->time0 + 0.5 * (cam->time1 - cam->time0);
  g.W = p->width, g.H = p->height;
  g.row_begin = p->row_begin, g.row_stride = p->row_stride, g.row_count = p->row_count;
  g.out = d_guides;
  return RTW_OK;
}
