// rtw_query_dev.hpp — the device pieces the ray-query kernels (rtw_query.hip)
// and the mirror-point kernels (rtw_specular.hip) share: a ray's and a hit
// record's layout in memory and the widening of a ray's box tests.
#pragma once
#include <hip/hip_runtime.h>

#include "rtw_device.hpp"
#include "rtw_world_walk.hpp"

namespace rtwk {

// rtw_ray: origin[3], dir[3], time, t_min, t_max (72 bytes, 8-byte loads).
struct QRay {
  V o, d;
  D time, tmin, tmax;
};
__device__ __forceinline__ QRay load_ray(const D* rays, uint64_t i) {
  const D* r = rays + 9 * i;
  QRay q;
  q.o = mk(r[0], r[1], r[2]);
  q.d = mk(r[3], r[4], r[5]);
  q.time = r[6], q.tmin = r[7], q.tmax = r[8];
  return q;
}
// rtw_hit: t, p[3], normal[3], u, v, {prim, front} (80 bytes, 8-byte stores); a miss is all zero.
__device__ __forceinline__ void store_hit(void* out, uint64_t i, D t, const HitRec& R, uint32_t prim) {
  D* h = static_cast<D*>(out) + 10 * i;
  h[0] = t;
  h[1] = R.p.x, h[2] = R.p.y, h[3] = R.p.z;
  h[4] = R.nrm.x, h[5] = R.nrm.y, h[6] = R.nrm.z;
  h[7] = R.u, h[8] = R.v;
  reinterpret_cast<uint64_t*>(h)[9] = (uint64_t)prim | ((uint64_t)(R.front ? 1u : 0u) << 32);
}
__device__ __forceinline__ void store_miss(void* out, uint64_t i) {
  uint64_t* h = static_cast<uint64_t*>(out) + 10 * i;
#pragma unroll
  for (int k = 0; k < 10; ++k) h[k] = 0ull;
}

// The widening of the ray's box tests: rtw_world_capi.hip bvh_margin with the
// ray's origin in the camera's place.
__device__ __forceinline__ D ray_margin(D reach, const V& o) {
  const D m = fmax(fmax(reach, fabs(o.x)), fmax(fabs(o.y), fabs(o.z)));
  const D L = 2.0 * m + 1.0;
  return 1e-7 * L + 0x1p-20 * L;
}

}  // namespace rtwk
