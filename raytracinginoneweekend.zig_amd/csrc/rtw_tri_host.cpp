// rtw_tri_host.cpp — the host reference of the triangle primitive (rtw_hip.h
// rtw_world_trace_tri_host): the reference's sequential list loop
// (HittableList.hit, hittable.zig:231-244) over a description's triangles only,
// each through its Translate / RotateY chain, with rtw_tri.hpp's root, inside
// test and hit record — the functions the kernels run.  What the device's
// records of triangle hits are compared with; no HIP here.
#include <cstdint>
#include <cstring>

#include "rtw_hip.h"
#include "rtw_tri.hpp"

int rtw_fail(int status, const char* fmt, ...);  // rtw_capi.hip: sets rtw_last_error

namespace {

struct V3 {
  double x, y, z;
};

// rtw_world_walk.hpp to_object / to_world over the description's chain (op 0 outermost).
void to_object(const rtw_xform& xf, V3& o, V3& d) {
  for (uint32_t i = 0; i < xf.n; ++i) {
    const double* v = xf.v[i];
    if (xf.op[i] == RTW_XF_TRANSLATE) {
      o.x = o.x - v[0], o.y = o.y - v[1], o.z = o.z - v[2];
    } else {
      const double sn = v[0], cs = v[1];
      const V3 o0 = o, d0 = d;
      o.x = cs * o0.x - sn * o0.z;
      o.z = sn * o0.x + cs * o0.z;
      d.x = cs * d0.x - sn * d0.z;
      d.z = sn * d0.x + cs * d0.z;
    }
  }
}
void to_world(const rtw_xform& xf, V3& p, V3& nrm) {
  for (int i = (int)xf.n - 1; i >= 0; --i) {
    const double* v = xf.v[i];
    if (xf.op[i] == RTW_XF_TRANSLATE) {
      p.x = p.x + v[0], p.y = p.y + v[1], p.z = p.z + v[2];
    } else {
      const double sn = v[0], cs = v[1];
      const V3 p0 = p, n0 = nrm;
      p.x = cs * p0.x + sn * p0.z;
      p.z = -sn * p0.x + cs * p0.z;
      nrm.x = cs * n0.x + sn * n0.z;
      nrm.z = -sn * n0.x + cs * n0.z;
    }
  }
}

}  // namespace

extern "C" int rtw_world_trace_tri_host(const rtw_world_desc* d, const rtw_ray* rays, size_t n,
                                        const rtw_query_opts* opts, rtw_hit* out) {
  const char* who = "rtw_world_trace_tri_host";
  if (!d || (n && (!rays || !out))) return rtw_fail(RTW_EINVAL, "%s: desc, rays or out is NULL", who);
  if ((d->n_prims && !d->prims) || (d->n_xforms && !d->xforms))
    return rtw_fail(RTW_EINVAL, "%s: NULL array with a non-zero count", who);
  if (opts && (opts->traversal > RTW_WORLD_TRAVERSAL_LANE || opts->flags != 0))
    return rtw_fail(RTW_EINVAL, "%s: opts.traversal %u / flags %u", who, opts->traversal, opts->flags);
  for (uint32_t i = 0; i < d->n_prims; ++i) {
    const rtw_prim& p = d->prims[i];
    if (p.kind != RTW_PRIM_TRIANGLE) continue;
    double nn[3], hh;
    bool fin = true;
    for (int k = 0; k < 9; ++k) fin = fin && p.a[k] - p.a[k] == 0.0;
    if (p.xform < -1 || p.xform >= (int32_t)d->n_xforms || !fin || !rtwtri::derive(p.a, nn, hh))
      return rtw_fail(RTW_EINVAL, "%s: prim %u: transform %d out of range, or a non-finite vertex or zero area", who, i,
                      p.xform);
    if (p.xform >= 0 && d->xforms[p.xform].n > RTW_MAX_XFORM_OPS)
      return rtw_fail(RTW_EINVAL, "%s: transform %d has %u ops", who, p.xform, d->xforms[p.xform].n);
  }
  for (size_t r = 0; r < n; ++r) {
    const rtw_ray& q = rays[r];
    double best = q.t_max;
    int64_t win = -1;
    for (uint32_t i = 0; i < d->n_prims; ++i) {
      const rtw_prim& p = d->prims[i];
      if (p.kind != RTW_PRIM_TRIANGLE) continue;
      V3 o{q.origin[0], q.origin[1], q.origin[2]}, dir{q.dir[0], q.dir[1], q.dir[2]};
      if (p.xform >= 0) to_object(d->xforms[p.xform], o, dir);
      double nv[3], h, t;
      (void)rtwtri::derive(p.a, nv, h);
      if (!rtwtri::root(p.a, nv[0], nv[1], nv[2], h, o.x, o.y, o.z, dir.x, dir.y, dir.z, q.t_min, t)) continue;
      if (best < t) continue;  // `t_max < root` rejects; a NaN root is accepted (as in the reference)
      best = t;
      win = (int64_t)i;
    }
    rtw_hit& H = out[r];
    std::memset(&H, 0, sizeof(H));
    if (win < 0) continue;
    const rtw_prim& p = d->prims[win];
    V3 o{q.origin[0], q.origin[1], q.origin[2]}, dir{q.dir[0], q.dir[1], q.dir[2]};
    if (p.xform >= 0) to_object(d->xforms[p.xform], o, dir);
    double nv[3], h;
    (void)rtwtri::derive(p.a, nv, h);
    V3 pt{o.x + dir.x * best, o.y + dir.y * best, o.z + dir.z * best};
    rtwtri::bary(p.a, o.x, o.y, o.z, dir.x, dir.y, dir.z, H.u, H.v);
    const bool front = nv[0] * dir.x + nv[1] * dir.y + nv[2] * dir.z < 0.0;
    V3 nrm = front ? V3{nv[0], nv[1], nv[2]} : V3{nv[0] * -1.0, nv[1] * -1.0, nv[2] * -1.0};
    if (p.xform >= 0) to_world(d->xforms[p.xform], pt, nrm);
    H.t = best;
    H.p[0] = pt.x, H.p[1] = pt.y, H.p[2] = pt.z;
    H.normal[0] = nrm.x, H.normal[1] = nrm.y, H.normal[2] = nrm.z;
    H.prim = (uint32_t)win + 1u;
    H.front = front ? 1u : 0u;
  }
  return RTW_OK;
}
