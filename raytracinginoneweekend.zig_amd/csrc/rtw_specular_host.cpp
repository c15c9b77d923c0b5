// rtw_specular_host.cpp — mirror points on the CPU (rtw_hip.h
// rtw_world_mirror_rays_host, rtw_world_mirror_points_host): rtw_specular.hpp's
// per-record functions over host buffers, as the device kernels
// (rtw_specular.hip) run them.  The library has no host tracer: the caller
// traces the reflected rays between the two calls.  No HIP here.  Also the
// argument check the host and device forms share.
#include <cstring>

#include "rtw_hip.h"
#include "rtw_specular.hpp"

int rtw_fail(int status, const char* fmt, ...);  // rtw_capi.hip: sets rtw_last_error

static_assert(sizeof(rtw_hit) == 80 && sizeof(rtw_ray) == 72 && sizeof(rtw_mirror_opts) == 8, "rtw_hip.h");
static_assert(RTW_MIRROR_PREDICT_ONLY == rtwsp::kPredictOnly && (uint32_t)RTW_WMAT_METAL == rtwsp::kMatMetal, "rtw_hip.h");

namespace rtwsp {

int check_call(const char* who, const void* rays, const void* hits, const void* hits2_in, uint64_t n,
               const void* cam_prev, const void* a_prev, size_t a_bytes, const void* xv_prev, size_t xv_bytes,
               uint32_t steps, uint32_t flags, const void* prev_p, const void* hits2_out, uint32_t& steps_out) {
  if (!cam_prev || !rays || !hits || !prev_p) return rtw_fail(RTW_EINVAL, "%s: cam_prev, rays, hits or prev_p is NULL", who);
  if (!resolve(steps, flags, steps_out))
    return rtw_fail(RTW_EINVAL, "%s: options out of range (steps %u of at most %u, flags 0x%x)", who, steps, kMaxSteps, flags);
  if ((((uintptr_t)rays | (uintptr_t)hits | (uintptr_t)hits2_in | (uintptr_t)prev_p | (uintptr_t)hits2_out |
        (uintptr_t)a_prev | (uintptr_t)xv_prev) & 7u) != 0)
    return rtw_fail(RTW_EINVAL, "%s: a buffer is not 8-byte aligned", who);
  // n <= 2^31 records of at most 80 bytes: nothing here wraps.
  struct Range {
    uintptr_t at;
    size_t bytes;
  };
  const Range out[2] = {{(uintptr_t)prev_p, (size_t)n * 24}, {(uintptr_t)hits2_out, (size_t)n * 80}};
  const Range in[6] = {{(uintptr_t)rays, (size_t)n * 72}, {(uintptr_t)hits, (size_t)n * 80}, {(uintptr_t)hits2_in, (size_t)n * 80},
                       {(uintptr_t)a_prev, a_bytes},      {(uintptr_t)xv_prev, xv_bytes},    {(uintptr_t)cam_prev, sizeof(rtw_camera)}};
  auto overlap = [](const Range& a, const Range& b) {
    return a.at && b.at && a.bytes && b.bytes && a.at < b.at + b.bytes && b.at < a.at + a.bytes;
  };
  for (const Range& o : out)
    for (const Range& i : in)
      if (overlap(o, i)) return rtw_fail(RTW_EINVAL, "%s: an output overlaps an input", who);
  if (overlap(out[0], out[1])) return rtw_fail(RTW_EINVAL, "%s: the two outputs overlap", who);
  return RTW_OK;
}

}  // namespace rtwsp

namespace {

int check_desc(const char* who, const rtw_world_desc* d) {
  if (!d) return rtw_fail(RTW_EINVAL, "%s: desc is NULL", who);
  if ((d->n_prims && !d->prims) || (d->n_xforms && !d->xforms) || (d->n_mats && !d->mats))
    return rtw_fail(RTW_EINVAL, "%s: NULL array with a non-zero count", who);
  for (uint32_t i = 0; i < d->n_prims; ++i)
    if (d->prims[i].kind == RTW_PRIM_TRIANGLE)
      return rtw_fail(RTW_UNSUPPORTED, "%s: primitive %u is a triangle: mirror points are not built for triangles", who, i);
  for (uint32_t i = 0; i < d->n_prims; ++i)
    if (d->prims[i].kind > RTW_PRIM_YZ_RECT || d->prims[i].xform < -1 || d->prims[i].xform >= (int32_t)d->n_xforms ||
        d->prims[i].mat >= d->n_mats)
      return rtw_fail(RTW_EINVAL, "%s: primitive %u: kind %u, transform %d, material %u", who, i, d->prims[i].kind,
                      d->prims[i].xform, d->prims[i].mat);
  for (uint32_t i = 0; i < d->n_xforms; ++i)
    if (d->xforms[i].n > RTW_MAX_XFORM_OPS) return rtw_fail(RTW_EINVAL, "%s: transform %u has %u ops", who, i, d->xforms[i].n);
  return RTW_OK;
}

bool record_is_mirror(const rtw_world_desc* d, const rtw_hit& h) {
  if (h.prim == 0u || h.prim > d->n_prims) return false;
  const rtw_prim& p = d->prims[h.prim - 1u];
  return rtwsp::is_mirror(h.prim, d->n_prims, h.front, p.kind, d->mats[p.mat].kind);
}

// What prev_point and prev_normal read of a primitive, as rtw_world_prev_points_host makes it.
struct PrimPrev {
  uint32_t kind, xf_h;
  double r[11];
  const double *v_now, *v_prev;
};
PrimPrev prim_prev(const rtw_world_desc* d, uint32_t prim, const double* a_prev, const double* xv_prev) {
  const rtw_prim& p = d->prims[prim - 1u];
  PrimPrev q;
  q.kind = p.kind, q.xf_h = 0u, q.v_now = nullptr, q.v_prev = nullptr;
  rtwr::fill_record(p.kind, a_prev ? a_prev + (size_t)9 * (prim - 1u) : p.a, q.r);
  if (p.xform >= 0) {
    const rtw_xform& x = d->xforms[p.xform];
    q.xf_h = x.n;
    for (uint32_t k = 0; k < x.n; ++k) q.xf_h |= (x.op[k] & 0xFu) << (8 + 4 * k);
    q.v_now = &x.v[0][0];
    q.v_prev = xv_prev ? xv_prev + (size_t)3 * RTW_MAX_XFORM_OPS * (size_t)p.xform : q.v_now;
  }
  return q;
}

}  // namespace

extern "C" {

int rtw_world_mirror_rays_host(const rtw_world_desc* d, const rtw_ray* rays, const rtw_hit* hits, uint64_t n,
                               rtw_ray* rays2, uint8_t* is_mirror) {
  const char* who = "rtw_world_mirror_rays_host";
  const int st = check_desc(who, d);
  if (st != RTW_OK) return st;
  if (n > RTW_QUERY_MAX_RAYS) return rtw_fail(RTW_EINVAL, "%s: n > 2^31", who);
  if (n == 0) return RTW_OK;
  if (!rays || !hits || !rays2 || !is_mirror) return rtw_fail(RTW_EINVAL, "%s: rays, hits, rays2 or is_mirror is NULL", who);
  if ((((uintptr_t)rays | (uintptr_t)hits | (uintptr_t)rays2) & 7u) != 0)
    return rtw_fail(RTW_EINVAL, "%s: a buffer is not 8-byte aligned", who);
  for (uint64_t i = 0; i < n; ++i) {
    const bool m = record_is_mirror(d, hits[i]);
    is_mirror[i] = m ? 1 : 0;
    if (m)
      rtwsp::reflect_ray(reinterpret_cast<const double*>(rays + i), hits[i].p, hits[i].normal,
                         reinterpret_cast<double*>(rays2 + i));
    else
      std::memset(rays2 + i, 0, sizeof(rtw_ray));
  }
  return RTW_OK;
}

int rtw_world_mirror_points_host(const rtw_world_desc* d, const rtw_ray* rays, const rtw_hit* hits, const rtw_hit* hits2,
                                 uint64_t n, const rtw_camera* cam_prev, const double* a_prev, const double* xv_prev,
                                 const rtw_mirror_opts* o, double* prev_p) {
  const char* who = "rtw_world_mirror_points_host";
  int st = check_desc(who, d);
  if (st != RTW_OK) return st;
  if (n > RTW_QUERY_MAX_RAYS) return rtw_fail(RTW_EINVAL, "%s: n > 2^31", who);
  const rtw_mirror_opts dflt{};
  if (!o) o = &dflt;
  if (n == 0) {
    uint32_t s0 = 0;
    if (!cam_prev || !rtwsp::resolve(o->steps, o->flags, s0)) return rtw_fail(RTW_EINVAL, "%s: cam_prev is NULL or options out of range", who);
    return RTW_OK;
  }
  if (!hits2) return rtw_fail(RTW_EINVAL, "%s: hits2 is NULL", who);
  uint32_t steps = 0;
  st = rtwsp::check_call(who, rays, hits, hits2, n, cam_prev, a_prev, (size_t)72 * d->n_prims, xv_prev,
                         (size_t)24 * RTW_MAX_XFORM_OPS * d->n_xforms, o->steps, o->flags, prev_p, nullptr, steps);
  if (st != RTW_OK) return st;
  const bool moved = a_prev || xv_prev;
  for (uint64_t i = 0; i < n; ++i) {
    const rtw_hit& h = hits[i];
    double* out = prev_p + 3 * i;
    if (h.prim == 0u || h.prim > d->n_prims) {
      out[0] = out[1] = out[2] = 0.0;
      continue;
    }
    const double time = rays[i].time;
    const PrimPrev q = prim_prev(d, h.prim, a_prev, xv_prev);
    double Mg[3];
    rtwt::prev_point(h.p, h.normal, h.u, h.v, h.front, q.kind, q.r, q.xf_h, q.v_now, q.v_prev, time, moved, Mg);
    if (!record_is_mirror(d, h)) {
      out[0] = Mg[0], out[1] = Mg[1], out[2] = Mg[2];
      continue;
    }
    double ng[3], r2[9], tg[3];
    rtwsp::prev_normal(h.normal, q.xf_h, q.v_now, q.v_prev, moved, ng);
    const rtw_hit& h2 = hits2[i];
    const bool tsky = h2.prim == 0u || h2.prim > d->n_prims;
    if (tsky) {
      rtwsp::reflect_ray(reinterpret_cast<const double*>(rays + i), h.p, h.normal, r2);
      const rtwsp::V3 u = rtwsp::unit(rtwsp::ld(r2 + 3));
      tg[0] = u.x, tg[1] = u.y, tg[2] = u.z;
    } else {
      const PrimPrev q2 = prim_prev(d, h2.prim, a_prev, xv_prev);
      rtwt::prev_point(h2.p, h2.normal, h2.u, h2.v, h2.front, q2.kind, q2.r, q2.xf_h, q2.v_now, q2.v_prev, time, moved, tg);
    }
    out[0] = Mg[0], out[1] = Mg[1], out[2] = Mg[2];
    double m[3];
    if (rtwsp::mirror_point(q.kind, Mg, ng, q.r[6], cam_prev->origin, tsky, tg, steps, m)) out[0] = m[0], out[1] = m[1], out[2] = m[2];
  }
  return RTW_OK;
}

}  // extern "C"
