// rtw_guides.hpp — what the two feature-buffer kernels share (rtw_guides.hip
// for scenes, rtw_world.hip for worlds): the pixel's feature ray and the
// record's store.  Device code; include after rtw_device.hpp.
#pragma once
#include "rtw_denoise.hpp"  // rtwd::Guide = rtw_guide
#include "rtw_device.hpp"

namespace rtwk {

// The lane's pixel: output row q (image row row_begin + q * row_stride), column x.
__device__ __forceinline__ bool guide_pixel(const GuideRay& G, uint32_t& x, uint32_t& q) {
  x = blockIdx.x * kGuideTileW + (threadIdx.x & (kGuideTileW - 1u));
  q = blockIdx.y * kGuideTileH + (threadIdx.x >> 6);
  return x < G.W && q < G.row_count;
}

// Camera.getRay (main.zig:91-100) with its draws at their means: s = (x + 0.5) /
// (W - 1), t = ((H - 1 - y) + 0.5) / (H - 1), no lens offset.
__device__ __forceinline__ void guide_ray(const GuideRay& G, uint32_t x, uint32_t q, V3<double>& o, V3<double>& d) {
  const uint32_t y = G.row_begin + q * G.row_stride;
  const double s = ((double)x + 0.5) / (double)(G.W - 1u);
  const double t = ((double)(G.H - 1u - y) + 0.5) / (double)(G.H - 1u);
  o = ld3(G.origin);
  d = sub(add(add(ld3(G.llc), mul(ld3(G.horizontal), s)), mul(ld3(G.vertical), t)), o);
}

__device__ __forceinline__ void guide_store(const GuideRay& G, uint32_t x, uint32_t q, const V3<double>& n, double depth,
                                            const V3<double>& albedo, uint32_t prim) {
  rtwd::Guide g;
  g.n[0] = (float)n.x, g.n[1] = (float)n.y, g.n[2] = (float)n.z;
  g.depth = (float)depth;
  g.albedo[0] = (float)albedo.x, g.albedo[1] = (float)albedo.y, g.albedo[2] = (float)albedo.z;
  g.prim = prim;
  static_cast<rtwd::Guide*>(G.out)[(size_t)q * G.W + x] = g;
}

}  // namespace rtwk
