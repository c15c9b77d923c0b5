// rtw_world_capi.hip — C ABI of the general-world path (include/rtw_hip.h
// "general worlds"): upload of the tables rtw_world_pack.cpp builds from an
// rtw_world_desc (validation, device records, BVH), and the render launches.
// Replaces the render loop of main.zig:378-402 for scenes 2-6 (and 1, 7).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "rtw_hip.h"
#include "rtw_capi_shared.hpp"
#include "rtw_internal.hpp"
#include "rtw_cull.hpp"
#include "rtw_denoise.hpp"
#include "rtw_host.hpp"
#include "rtw_libm.hpp"
#include "rtw_orbit.hpp"
#include "rtw_specular.hpp"
#include "rtw_world_pack.hpp"
#include "rtw_world_rebuild.hpp"
#include "rtw_world_update.hpp"

struct rtw_world_s {
  int device = 0;
  void* buf = nullptr;
  rtwk::WorldView view{};
  double bounds_lo[3] = {0, 0, 0}, bounds_hi[3] = {0, 0, 0};  // box of every primitive (+-inf when empty)
  bool has_moving = false;
  uint32_t feat = 0;  // features used (rtw_world.hip kFeat*): picks the kernel instantiation
  uint32_t info[4] = {0, 0, 0, 0};
  bool packed = false;  // the BVH carries the refs in its bounds' low bits (rtw_world_pack.cpp pack_refs)
  size_t table_bytes = 0;  // of buf
  uint32_t n_xforms = 0;   // transform chains of the description
  // RTW_WORLD_DYNAMIC (rtw_hip.h "dynamic worlds"): the refit's tables, the validation's partials and
  // the host entry's staging arrays in a second allocation; nullptr for a frozen world
  rtwp::RefitPack* refit = nullptr;
  void* refit_buf = nullptr;
  rtwk::UpdateArgs upd{};  // device pointers of both allocations (a / xv: per call)
  double* stage_a = nullptr;
  double* stage_xv = nullptr;
  // rtw_world_rebuild*: keys, sort storage, the staged topology (made at the first rebuild and kept)
  void* rebuild_buf = nullptr;
  rtwk::RebuildArgs reb{};
  // rtw_world_bvh_cost: per-workgroup partials and the result (made at the first call and kept)
  double* cost_buf = nullptr;
};

namespace {
// The second allocation of a DYNAMIC world: RefitPack::blob | partials | result | staging a | staging xv.
int make_dynamic(rtw_world_s* w, const rtw_world_desc* d, const rtwp::WorldPack& k) {
  auto* r = new rtwp::RefitPack;
  rtwp::make_refit(d, k, *r);
  const uint32_t n_wg = std::max(1u, (std::max(k.n_prims, d->n_xforms) + rtwr::kBlock - 1) / rtwr::kBlock);
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_part = r->blob.size(), o_res = o_part + al((size_t)n_wg * rtwr::kPartial * 8),
               o_a = o_res + al(rtwr::kPartial * 8), o_xv = o_a + al((size_t)k.n_prims * 9 * 8 + 8),
               total = o_xv + al((size_t)d->n_xforms * 3 * RTW_MAX_XFORM_OPS * 8 + 8);
  void* buf = nullptr;
  if (hipMalloc(&buf, total) != hipSuccess) {
    delete r;
    return rtw_fail(RTW_ENOMEM, "rtw_world_create: hipMalloc(%zu) for the refit tables", total);
  }
  if (hipMemset(buf, 0, total) != hipSuccess ||
      hipMemcpy(buf, r->blob.data(), r->blob.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(buf);
    delete r;
    return rtw_fail(RTW_EHIP, "rtw_world_create: upload of the refit tables failed");
  }
  auto* rb = static_cast<unsigned char*>(buf);
  rtwr::View& V = w->upd.v;
  V.prim = const_cast<double*>(w->view.prim), V.xform = const_cast<double*>(w->view.xform);
  V.node = const_cast<float*>(w->view.node), V.order = w->view.order, V.cull = const_cast<float*>(w->view.cull);
  V.by_height = reinterpret_cast<const uint32_t*>(rb + r->o_by_height);
  V.heights = reinterpret_cast<const uint32_t*>(rb + r->o_heights);
  V.plain = reinterpret_cast<float*>(rb + r->o_plain);
  V.cand = reinterpret_cast<const uint32_t*>(rb + r->o_cand);
  V.mate = reinterpret_cast<const uint32_t*>(rb + r->o_mate);
  V.n_prims = k.n_prims, V.n_xforms = d->n_xforms, V.n_nodes = k.n_nodes;
  V.packed = k.packed ? 1u : 0u, V.has_table = k.has_cull ? 1u : 0u;
  V.has_tri = (k.feat & 64u) ? 1u : 0u;
  w->upd.partials = reinterpret_cast<double*>(rb + o_part);
  w->upd.result = reinterpret_cast<double*>(rb + o_res);
  w->upd.n_wg = n_wg;
  w->stage_a = reinterpret_cast<double*>(rb + o_a);
  w->stage_xv = reinterpret_cast<double*>(rb + o_xv);
  r->blob = std::vector<unsigned char>();  // (the device holds it now)
  w->refit = r;
  w->refit_buf = buf;
  return RTW_OK;
}
}  // namespace

extern "C" {

int rtw_world_create(const rtw_world_desc* d, uint32_t flags, rtw_world* out) {
  if (!out || !d) return rtw_fail(RTW_EINVAL, "rtw_world_create: desc/out is NULL");
  *out = nullptr;
  const char* nc = rtw_dev_knob("RTW_WORLD_NOCULL");  // development knob (A/B): no leaf pretest
  rtwp::WorldPack k;
  std::string msg;
  const int st = rtwp::pack_world(d, flags, nc && *nc, k, msg);
  if (st != RTW_OK) return rtw_fail(st, "%s", msg.c_str());
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return rtw_fail(RTW_ENODEV, "no HIP device");
  const size_t total = k.blob.size();
  void* buf = nullptr;
  if (hipMalloc(&buf, total) != hipSuccess) return rtw_fail(RTW_ENOMEM, "rtw_world_create: hipMalloc(%zu)", total);
  if (hipMemcpy(buf, k.blob.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(buf);
    return rtw_fail(RTW_EHIP, "rtw_world_create: hipMemcpy failed");
  }
  rtw_world_s* w = new rtw_world_s;
  auto* base = static_cast<unsigned char*>(buf);
  w->device = dev;
  w->buf = buf;
  w->view.prim = reinterpret_cast<const double*>(base + k.o_prim);
  w->view.xform = reinterpret_cast<const double*>(base + k.o_xform);
  w->view.tex = reinterpret_cast<const double*>(base + k.o_tex);
  w->view.mat = reinterpret_cast<const double*>(base + k.o_mat);
  w->view.perlin = reinterpret_cast<const double*>(base + k.o_perlin);
  w->view.image = reinterpret_cast<const uint32_t*>(base + k.o_image);
  w->view.pixels = base + k.o_pixels;
  w->view.node = reinterpret_cast<const float*>(base + k.o_node);
  w->view.order = reinterpret_cast<const uint32_t*>(base + k.o_order);
  w->view.cull = reinterpret_cast<const float*>(base + k.o_cull);
  w->view.n_prims = k.n_prims;
  w->view.n_nodes = k.n_nodes;
  w->view.n_perlins = k.n_perlins;
  w->view.flags = k.view_flags;
  w->view.cull_cmax = k.cull_cmax;
  w->view.cull_rho = k.cull_rho;
  std::memcpy(w->bounds_lo, k.bounds_lo, sizeof(w->bounds_lo));
  std::memcpy(w->bounds_hi, k.bounds_hi, sizeof(w->bounds_hi));
  w->has_moving = k.has_moving;
  w->feat = k.feat;
  std::memcpy(w->info, k.info, sizeof(w->info));
  w->packed = k.packed;
  w->table_bytes = total;
  w->n_xforms = d->n_xforms;
  if (flags & RTW_WORLD_DYNAMIC) {
    const int sd = make_dynamic(w, d, k);
    if (sd != RTW_OK) {
      (void)hipFree(buf);
      delete w;
      return sd;
    }
  }
  *out = w;
  return RTW_OK;
}

int rtw_world_destroy(rtw_world w) {
  if (!w) return RTW_OK;
  if (w->buf) (void)hipFree(w->buf);
  if (w->refit_buf) (void)hipFree(w->refit_buf);
  if (w->rebuild_buf) (void)hipFree(w->rebuild_buf);
  if (w->cost_buf) (void)hipFree(w->cost_buf);
  delete w->refit;
  delete w;
  return RTW_OK;
}

int rtw_world_update_device(rtw_world w, const double* d_a, const double* d_xv, void* stream) {
  if (!w) return rtw_fail(RTW_EINVAL, "rtw_world_update_device: world is NULL");
  if (!w->refit) return rtw_fail(RTW_EINVAL, "rtw_world_update_device: the world was not created with RTW_WORLD_DYNAMIC");
  if (!d_a && w->view.n_prims) return rtw_fail(RTW_EINVAL, "rtw_world_update_device: d_a is NULL");
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return rtw_fail(RTW_ENODEV, "no HIP device");
  if (dev != w->device)
    return rtw_fail(RTW_EINVAL, "rtw_world_update_device: world lives on device %d, current is %d", w->device, dev);
  hipStream_t s = static_cast<hipStream_t>(stream);
  rtwk::UpdateArgs a = w->upd;
  a.v.a = d_a ? d_a : w->stage_a, a.v.xv = d_xv;
  // validate: reads the input only; the one readback the host waits for
  hipError_t e = rtwk::launch_update_validate(a, s);
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "update validation launch: %s", hipGetErrorString(e));
  double res[rtwr::kPartial];
  HIP_TRY(hipMemcpyAsync(res, a.result, sizeof(res), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  rtwr::Partial p;
  rtwr::partial_load(p, res);
  if (p.bad != 0.0)
    return rtw_fail(RTW_EINVAL, "rtw_world_%s", rtwp::refit_violation(p.bad, p.first_bad, w->view.n_prims).c_str());
  // commit
  rtwp::refit_scalars(p, w->view.n_nodes, w->view.cull_cmax, w->view.cull_rho, w->bounds_lo, w->bounds_hi);
  a.v.cull_on = (a.v.has_table && w->view.cull_cmax <= rtwc::kCmaxLimit) ? 1u : 0u;
  e = rtwk::launch_update_commit(a, w->refit->h_off.data(), w->refit->h_max, w->refit->h_star, s);
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "update commit launch: %s", hipGetErrorString(e));
  return RTW_OK;
}

int rtw_world_update(rtw_world w, const rtw_prim* prims, uint32_t n_prims, const rtw_xform* xforms, uint32_t n_xforms) {
  if (!w) return rtw_fail(RTW_EINVAL, "rtw_world_update: world is NULL");
  if (!w->refit) return rtw_fail(RTW_EINVAL, "rtw_world_update: the world was not created with RTW_WORLD_DYNAMIC");
  if ((n_prims && !prims) || (n_xforms && !xforms)) return rtw_fail(RTW_EINVAL, "rtw_world_update: NULL array with a non-zero count");
  std::string msg;
  if (!rtwp::same_fixed_fields(*w->refit, prims, n_prims, xforms, n_xforms, msg))
    return rtw_fail(RTW_EINVAL, "rtw_world_update: %s", msg.c_str());
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return rtw_fail(RTW_ENODEV, "no HIP device");
  if (dev != w->device) return rtw_fail(RTW_EINVAL, "rtw_world_update: world lives on device %d, current is %d", w->device, dev);
  std::vector<double> a((size_t)9 * n_prims), xv((size_t)3 * RTW_MAX_XFORM_OPS * n_xforms);
  for (uint32_t i = 0; i < n_prims; ++i) std::memcpy(a.data() + (size_t)9 * i, prims[i].a, sizeof(prims[i].a));
  for (uint32_t i = 0; i < n_xforms; ++i) std::memcpy(xv.data() + (size_t)12 * i, xforms[i].v, sizeof(xforms[i].v));
  // (the null stream: an earlier update's kernels have read the staging arrays before these copies land)
  if (!a.empty()) HIP_TRY(hipMemcpy(w->stage_a, a.data(), a.size() * 8, hipMemcpyHostToDevice));
  if (!xv.empty()) HIP_TRY(hipMemcpy(w->stage_xv, xv.data(), xv.size() * 8, hipMemcpyHostToDevice));
  return rtw_world_update_device(w, w->stage_a, n_xforms ? w->stage_xv : nullptr, nullptr);
}

}  // extern "C"

namespace {
// The third allocation of a DYNAMIC world, made at its first rebuild and kept:
// self | partials | readback | centroid partials | centroid box | keys x 2 | sorted | ranges | refs |
// schedule x 2 | meta | the sort's storage.
int make_rebuild(rtw_world_s* w, hipStream_t s) {
  const uint32_t n = w->view.n_prims, nn = w->view.n_nodes, n_wg = w->upd.n_wg;
  size_t sort_bytes = 0;
  if (rtwk::rebuild_sort_bytes(n, &sort_bytes) != hipSuccess)
    return rtw_fail(RTW_EHIP, "rtw_world_rebuild: the sort's storage size");
  size_t total = 0;
  auto take = [&](size_t b) {
    const size_t o = total;
    total += (std::max(b, (size_t)8) + 255) & ~(size_t)255;
    return o;
  };
  const size_t o_self = take((size_t)n * 4), o_part = take((size_t)n_wg * rtwr::kPartial * 8),
               o_read = take(rtwb::kReadbackBytes), o_cpart = take((size_t)n_wg * 6 * 8), o_cbox = take(6 * 8),
               o_key = take((size_t)n * 8), o_keys = take((size_t)n * 8), o_sorted = take((size_t)n * 4),
               o_rng = take((size_t)nn * 8), o_refs = take((size_t)nn * 8), o_byh = take((size_t)nn * 4),
               o_hts = take((size_t)nn * 4), o_meta = take((size_t)n * 24), o_sort = take(sort_bytes);
  void* buf = nullptr;
  if (hipMalloc(&buf, total) != hipSuccess) return rtw_fail(RTW_ENOMEM, "rtw_world_rebuild: hipMalloc(%zu) for the rebuild", total);
  if (hipMemsetAsync(buf, 0, total, s) != hipSuccess) {
    (void)hipFree(buf);
    return rtw_fail(RTW_EHIP, "rtw_world_rebuild: clearing the rebuild allocation failed");
  }
  auto* b = static_cast<unsigned char*>(buf);
  rtwk::RebuildArgs& a = w->reb;
  a.v = w->upd.v;
  a.self = reinterpret_cast<uint32_t*>(b + o_self);
  a.partials = reinterpret_cast<double*>(b + o_part);
  a.result = reinterpret_cast<double*>(b + o_read);
  a.levels = reinterpret_cast<uint32_t*>(b + o_read + rtwr::kPartial * 8);
  a.cpart = reinterpret_cast<double*>(b + o_cpart);
  a.cbox = reinterpret_cast<double*>(b + o_cbox);
  a.key = reinterpret_cast<uint64_t*>(b + o_key);
  a.keys = reinterpret_cast<uint64_t*>(b + o_keys);
  a.sorted = reinterpret_cast<uint32_t*>(b + o_sorted);
  a.rng = reinterpret_cast<uint32_t*>(b + o_rng);
  a.refs = reinterpret_cast<uint32_t*>(b + o_refs);
  a.by_height = reinterpret_cast<uint32_t*>(b + o_byh);
  a.heights = reinterpret_cast<uint32_t*>(b + o_hts);
  a.meta = reinterpret_cast<double*>(b + o_meta);
  a.sort_tmp = b + o_sort;
  a.sort_bytes = sort_bytes;
  a.n_wg = n_wg;
  w->rebuild_buf = buf;
  const hipError_t e = rtwk::launch_rebuild_init(a, s);
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "rebuild init launch: %s", hipGetErrorString(e));
  return RTW_OK;
}
}  // namespace

extern "C" {

int rtw_world_rebuild_device(rtw_world w, const double* d_a, const double* d_xv, void* stream) {
  if (!w) return rtw_fail(RTW_EINVAL, "rtw_world_rebuild_device: world is NULL");
  if (!w->refit) return rtw_fail(RTW_EINVAL, "rtw_world_rebuild_device: the world was not created with RTW_WORLD_DYNAMIC");
  if (!rtwp::rebuild_supported(w->view.n_prims, w->view.n_nodes, w->info))
    return rtw_fail(RTW_UNSUPPORTED, "rtw_world_rebuild_device: the world has no BVH with leaves of one primitive");
  if (!d_a) return rtw_fail(RTW_EINVAL, "rtw_world_rebuild_device: d_a is NULL");
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return rtw_fail(RTW_ENODEV, "no HIP device");
  if (dev != w->device)
    return rtw_fail(RTW_EINVAL, "rtw_world_rebuild_device: world lives on device %d, current is %d", w->device, dev);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!w->rebuild_buf) {
    const int st = make_rebuild(w, s);
    if (st != RTW_OK) return st;
  }
  rtwk::RebuildArgs r = w->reb;
  r.v.a = d_a, r.v.xv = d_xv;
  // phase 1 reads the input and the world, and writes the rebuild allocation only: the validation with
  // every primitive its own mate (a leaf of one is judged on its own sphere), then keys, sort and topology
  rtwk::UpdateArgs va = w->upd;
  va.v = r.v, va.v.mate = r.self, va.partials = r.partials, va.result = r.result;
  hipError_t e = rtwk::launch_update_validate(va, s);
  if (e == hipSuccess) e = rtwk::launch_rebuild_build(r, s);
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "rebuild launch: %s", hipGetErrorString(e));
  // the one readback the host waits for: the partial, the depth, the nodes per level
  alignas(8) unsigned char back[rtwb::kReadbackBytes];
  HIP_TRY(hipMemcpyAsync(back, r.result, sizeof(back), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  rtwr::Partial p;
  rtwr::partial_load(p, reinterpret_cast<const double*>(back));
  if (p.bad != 0.0)
    return rtw_fail(RTW_EINVAL, "rtw_world_%s", rtwp::refit_violation(p.bad, p.first_bad, w->view.n_prims).c_str());
  uint32_t levels[1 + rtwb::kMaxLevels];
  std::memcpy(levels, back + rtwr::kPartial * 8, sizeof(levels));
  const uint32_t depth = levels[0];
  uint32_t sum = 0;
  for (uint32_t l = 0; l < depth && l < rtwb::kMaxLevels; ++l) sum += levels[1 + l];
  if (depth == 0 || depth > rtwb::cap_of(w->view.n_prims) || sum != w->view.n_nodes)
    return rtw_fail(RTW_EHIP, "rtw_world_rebuild_device: the device built %u levels of %u nodes", depth, sum);
  // commit: the new topology, then the update's commit over it
  rtwp::level_schedule(levels + 1, depth, w->view.n_nodes, *w->refit);
  w->info[2] = depth;
  rtwp::refit_scalars(p, w->view.n_nodes, w->view.cull_cmax, w->view.cull_rho, w->bounds_lo, w->bounds_hi);
  r.v.cull_on = (r.v.has_table && w->view.cull_cmax <= rtwc::kCmaxLimit) ? 1u : 0u;
  e = rtwk::launch_rebuild_apply(r, s);
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "rebuild apply launch: %s", hipGetErrorString(e));
  rtwk::UpdateArgs ca = w->upd;
  ca.v = r.v;
  e = rtwk::launch_update_commit(ca, w->refit->h_off.data(), w->refit->h_max, w->refit->h_star, s);
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "rebuild commit launch: %s", hipGetErrorString(e));
  return RTW_OK;
}

int rtw_world_rebuild(rtw_world w, const rtw_prim* prims, uint32_t n_prims, const rtw_xform* xforms, uint32_t n_xforms) {
  if (!w) return rtw_fail(RTW_EINVAL, "rtw_world_rebuild: world is NULL");
  if (!w->refit) return rtw_fail(RTW_EINVAL, "rtw_world_rebuild: the world was not created with RTW_WORLD_DYNAMIC");
  if (!rtwp::rebuild_supported(w->view.n_prims, w->view.n_nodes, w->info))
    return rtw_fail(RTW_UNSUPPORTED, "rtw_world_rebuild: the world has no BVH with leaves of one primitive");
  if ((n_prims && !prims) || (n_xforms && !xforms)) return rtw_fail(RTW_EINVAL, "rtw_world_rebuild: NULL array with a non-zero count");
  std::string msg;
  if (!rtwp::same_fixed_fields(*w->refit, prims, n_prims, xforms, n_xforms, msg))
    return rtw_fail(RTW_EINVAL, "rtw_world_rebuild: %s", msg.c_str());
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return rtw_fail(RTW_ENODEV, "no HIP device");
  if (dev != w->device) return rtw_fail(RTW_EINVAL, "rtw_world_rebuild: world lives on device %d, current is %d", w->device, dev);
  std::vector<double> a((size_t)9 * n_prims), xv((size_t)3 * RTW_MAX_XFORM_OPS * n_xforms);
  for (uint32_t i = 0; i < n_prims; ++i) std::memcpy(a.data() + (size_t)9 * i, prims[i].a, sizeof(prims[i].a));
  for (uint32_t i = 0; i < n_xforms; ++i) std::memcpy(xv.data() + (size_t)12 * i, xforms[i].v, sizeof(xforms[i].v));
  // (the null stream, as rtw_world_update)
  if (!a.empty()) HIP_TRY(hipMemcpy(w->stage_a, a.data(), a.size() * 8, hipMemcpyHostToDevice));
  if (!xv.empty()) HIP_TRY(hipMemcpy(w->stage_xv, xv.data(), xv.size() * 8, hipMemcpyHostToDevice));
  return rtw_world_rebuild_device(w, w->stage_a, n_xforms ? w->stage_xv : nullptr, nullptr);
}

int rtw_world_bvh_cost(rtw_world w, void* stream, double* cost_out) {
  if (!w || !cost_out) return rtw_fail(RTW_EINVAL, "rtw_world_bvh_cost: world/cost_out is NULL");
  if (!w->view.n_nodes) return rtw_fail(RTW_UNSUPPORTED, "rtw_world_bvh_cost: the world has no BVH");
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return rtw_fail(RTW_ENODEV, "no HIP device");
  if (dev != w->device) return rtw_fail(RTW_EINVAL, "rtw_world_bvh_cost: world lives on device %d, current is %d", w->device, dev);
  const uint32_t wg = (w->view.n_nodes + rtwr::kBlock - 1) / rtwr::kBlock;
  if (!w->cost_buf && hipMalloc(reinterpret_cast<void**>(&w->cost_buf), ((size_t)wg + 1) * 8) != hipSuccess)
    return rtw_fail(RTW_ENOMEM, "rtw_world_bvh_cost: hipMalloc");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const hipError_t e = rtwk::launch_bvh_cost(w->view.node, w->view.n_nodes, w->cost_buf + 1, w->cost_buf, s);
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "tree cost launch: %s", hipGetErrorString(e));
  HIP_TRY(hipMemcpyAsync(cost_out, w->cost_buf, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return RTW_OK;
}

int rtw_world_rebuild_tables_host(const rtw_world_desc* d, uint32_t flags, const double* a, const double* xv, void* out,
                                  size_t bytes, float cull_out[2], double bounds_out[6], uint32_t info_out[4]) {
  return rtw_world_rebuild_refit_tables_host(d, flags, a, xv, nullptr, nullptr, out, bytes, cull_out, bounds_out, info_out);
}

int rtw_world_rebuild_refit_tables_host(const rtw_world_desc* d, uint32_t flags, const double* a, const double* xv,
                                        const double* a2, const double* xv2, void* out, size_t bytes, float cull_out[2],
                                        double bounds_out[6], uint32_t info_out[4]) {
  if (!d || !out || !a) return rtw_fail(RTW_EINVAL, "rtw_world_rebuild_tables_host: desc/out/a is NULL");
  const char* nc = rtw_dev_knob("RTW_WORLD_NOCULL");  // (as rtw_world_create)
  rtwp::WorldPack k;
  std::string msg;
  const int st = rtwp::pack_world(d, flags, nc && *nc, k, msg);
  if (st != RTW_OK) return rtw_fail(st, "%s", msg.c_str());
  if (bytes != k.blob.size()) return rtw_fail(RTW_EINVAL, "rtw_world_rebuild_tables_host: %zu bytes, the tables have %zu", bytes, k.blob.size());
  rtwp::RefitPack r;
  rtwp::make_refit(d, k, r);
  const int sb = rtwp::rebuild_world(k, r, a, xv);
  if (sb != RTW_OK) return rtw_fail(sb, "rtw_world_%s", r.msg.c_str());
  if (rtwp::refit_world(k, r, a, xv) != RTW_OK) return rtw_fail(RTW_EINVAL, "rtw_world_%s", r.msg.c_str());
  if (a2 && rtwp::refit_world(k, r, a2, xv2) != RTW_OK) return rtw_fail(RTW_EINVAL, "rtw_world_%s", r.msg.c_str());
  std::memcpy(out, k.blob.data(), bytes);
  if (cull_out) cull_out[0] = k.cull_cmax, cull_out[1] = k.cull_rho;
  if (bounds_out)
    for (int c = 0; c < 3; ++c) bounds_out[c] = k.bounds_lo[c], bounds_out[3 + c] = k.bounds_hi[c];
  if (info_out) std::memcpy(info_out, k.info, sizeof(k.info));
  return RTW_OK;
}

size_t rtw_world_table_bytes(rtw_world w) { return w ? w->table_bytes : 0; }

int rtw_world_read_tables(rtw_world w, void* out, size_t bytes, float cull_out[2], double bounds_out[6]) {
  if (!w || !out) return rtw_fail(RTW_EINVAL, "rtw_world_read_tables: world/out is NULL");
  if (bytes != w->table_bytes) return rtw_fail(RTW_EINVAL, "rtw_world_read_tables: %zu bytes, the tables have %zu", bytes, w->table_bytes);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, w->buf, bytes, hipMemcpyDeviceToHost));
  if (cull_out) cull_out[0] = w->view.cull_cmax, cull_out[1] = w->view.cull_rho;
  if (bounds_out)
    for (int c = 0; c < 3; ++c) bounds_out[c] = w->bounds_lo[c], bounds_out[3 + c] = w->bounds_hi[c];
  return RTW_OK;
}

int rtw_world_refit_tables_host(const rtw_world_desc* d, uint32_t flags, const double* a, const double* xv, void* out,
                                size_t bytes, float cull_out[2], double bounds_out[6]) {
  if (!d || !out) return rtw_fail(RTW_EINVAL, "rtw_world_refit_tables_host: desc/out is NULL");
  const char* nc = rtw_dev_knob("RTW_WORLD_NOCULL");  // (as rtw_world_create)
  rtwp::WorldPack k;
  std::string msg;
  const int st = rtwp::pack_world(d, flags, nc && *nc, k, msg);
  if (st != RTW_OK) return rtw_fail(st, "%s", msg.c_str());
  if (bytes != k.blob.size()) return rtw_fail(RTW_EINVAL, "rtw_world_refit_tables_host: %zu bytes, the tables have %zu", bytes, k.blob.size());
  if (a || xv) {
    if (!a && d->n_prims) return rtw_fail(RTW_EINVAL, "rtw_world_refit_tables_host: xv without a");
    rtwp::RefitPack r;
    rtwp::make_refit(d, k, r);
    if (rtwp::refit_world(k, r, a, xv) != RTW_OK) return rtw_fail(RTW_EINVAL, "rtw_world_%s", r.msg.c_str());
  }
  std::memcpy(out, k.blob.data(), bytes);
  if (cull_out) cull_out[0] = k.cull_cmax, cull_out[1] = k.cull_rho;
  if (bounds_out)
    for (int c = 0; c < 3; ++c) bounds_out[c] = k.bounds_lo[c], bounds_out[3 + c] = k.bounds_hi[c];
  return RTW_OK;
}

int rtw_world_bvh_info(rtw_world w, uint32_t info_out[4]) {
  if (!w || !info_out) return rtw_fail(RTW_EINVAL, "world/info is NULL");
  std::memcpy(info_out, w->info, sizeof(w->info));
  return RTW_OK;
}

}  // extern "C"

namespace {

// Default register-allocation target (waves per SIMD) from the A/Bs on MI355X
// (DESIGN.md §6.3): 4 waves hide the BVH's dependent node loads; worlds with
// rects or transforms (the Cornell box) run 2 % faster at the 3-wave budget
// since round 4's register work (profiles/r04/world_occ_ab.txt; round 1: 4 was
// best); Perlin-textured worlds keep the 2-wave budget because their noise
// loops spill badly.
static_assert(rtwk::kMaxXfOps == RTW_MAX_XFORM_OPS, "transform chain length");
int world_occ_default(const rtw_world_s* w) {
  if (w->view.n_perlins) return 1;
  // rtw_world.hip kFeatXform | kFeatRect; kFeatTri: at the 4-wave budget (128 VGPRs) every triangle set
  // spills (64-128 B per lane; per lane too, the record is 13 doubles), at 3 waves none does, and the mesh
  // world of tools/mesh_bench.py renders 10 % faster there (profiles/r26/mesh.txt)
  return (w->feat & (4u | 8u | 64u)) ? 3 : 4;
}

// Widening of every BVH box test.  A computed sphere root deviates from the
// exact intersection by at most ~sqrt(u * (hb^2 + |a c|)) / a (u = 2^-53; the
// sqrt of a discriminant with absolute error u*(hb^2 + |ac|)), i.e. in space
// by <= sqrt(u) * sqrt(2 |o - c|^2 + r^2) <= 2.2e-8 * L, where L bounds
// |o - c| + r over every ray origin o (camera or a surface point) and
// primitive.  Rect roots and the slab arithmetic are accurate to a few u * L.
// margin = 1e-7 * L with L = 2 * (max |coordinate| of the scene box and the
// camera) + 1 covers both with a 4x safety factor.  The kernel evaluates the
// slabs in packed f32 (t = fma(b, RN(1/d), RN(-RN(o) RN(1/d)))): expressed in
// space, its rounding is <= 4 u32 (|o| + |b|) <= 2^-22 L (u32 = 2^-24; the
// f32 bounds are rounded outward), so 2^-20 L more (4x) is added.  A box
// that holds a primitive the linear list would accept is never pruned.
double bvh_margin(const rtw_world_s* w, const rtw_camera* cam) {
  double m = 0;
  for (int k = 0; k < 3; ++k) {
    if (std::isfinite(w->bounds_lo[k])) m = std::max(m, std::fabs(w->bounds_lo[k]));
    if (std::isfinite(w->bounds_hi[k])) m = std::max(m, std::fabs(w->bounds_hi[k]));
    m = std::max(m, std::fabs(cam->origin[k]) + cam->lens_radius * 2);
  }
  const double L = 2.0 * m + 1.0;
  return 1e-7 * L + 0x1p-20 * L;
}

// The launch configuration of a world render on device `dev`: kernel
// instantiation (feature set), register budget, LDS, persistent grid, and the
// tail dealing's ring bytes (one kTailWin-entry f64x3 ring per lane of the
// grid, WorldArgs::ring), which live in the caller's workspace after the
// common region (rtwp::world_ring_off), so renders on different streams with their
// own workspaces never share one.
struct WorldLaunchCfg {
  int fs, oi, bpc;
  size_t lds;
  uint32_t grid;
  size_t ring_off, ring_bytes;  // ring: [ring_off, ring_off + ring_bytes) of the workspace
};
constexpr uint32_t kLaneYield = 16;   // (A/B of RTW_WORLD_YIELD 12 / 16 / 24 / 32: profiles/r05/world_lane_ab.txt)
constexpr uint32_t kLaneNodes = 256;  // AUTO traversal: per lane from this BVH size on
WorldLaunchCfg world_cfg(const rtw_world_s* w, const rtw_params* p, int dev) {
  WorldLaunchCfg c;
  // Kernel instantiation for the world's features (params.world_features
  // RTW_WORLD_FEATURES_ALL: the general kernel; every set gives the same bits)
  // and its BVH traversal (params.world_traversal): per lane for sphere worlds
  // whose BVH fits the per-lane stack, else the wave's union walk.
  const uint32_t feat = p->world_features == RTW_WORLD_FEATURES_ALL ? (15u | (w->feat & 64u)) : w->feat;  // (64: kFeatTri)
  // AUTO: per lane on BVHs of >= kLaneNodes nodes (configs[4]'s globe: 5,802
  // nodes, +30 %); the union walk on small trees, where the lanes' paths
  // mostly coincide (scene 1's 23 nodes: the union 17 % faster).
  const bool lane_ok = w->view.n_nodes > 0 && w->info[2] <= rtwk::kLaneStack && w->info[3] <= rtwk::kMaxLeafPrims &&
                       w->view.n_prims + 1u < (1u << rtwk::kTravPosBits) && (feat & ~(2u | 64u)) == 0u;
  const bool lane = lane_ok && (p->world_traversal == RTW_WORLD_TRAVERSAL_LANE ||
                                (p->world_traversal == RTW_WORLD_TRAVERSAL_AUTO && w->view.n_nodes >= kLaneNodes));
  const char* up = rtw_dev_knob("RTW_WORLD_UNPACKED");  // development knob (A/B): the per-lane walk loads the refs
  const bool packed = lane && w->packed && !(up && *up == '1');
  c.fs = rtwk::world_feature_set(feat, lane, packed);
  c.lds = rtwk::world_lds_bytes(w->view.n_perlins, c.fs);
  // Register-allocation target in waves per SIMD (params.world_waves, 0 = the
  // feature set's default).
  const int occ = p->world_waves ? (int)p->world_waves : world_occ_default(w);
  c.oi = occ >= 4 ? 4 : (occ == 3 ? 3 : 1);
  static std::mutex mu;
  static int bpc_cache[128][5] = {};
  static size_t bpc_lds[128][5] = {};
  int bpc;
  {
    std::lock_guard<std::mutex> lk(mu);
    if (bpc_cache[c.fs][c.oi] == 0 || bpc_lds[c.fs][c.oi] != c.lds)
      bpc_cache[c.fs][c.oi] = rtwk::world_blocks_per_cu(c.lds, c.oi, c.fs), bpc_lds[c.fs][c.oi] = c.lds;
    bpc = bpc_cache[c.fs][c.oi];
  }
  c.bpc = bpc;
  const uint32_t want = ((uint32_t)rtwp::total_units(p) + 255) / 256;
  c.grid = std::max(1u, std::min((uint32_t)(rtw_device_cus(dev) * bpc), want));
  c.ring_off = rtwp::world_ring_off(p);
  c.ring_bytes = (size_t)c.grid * rtwk::kWorldBlock * rtwk::kTailWin * 3 * sizeof(double);
  return c;
}

int world_launch(rtw_world w, const rtw_camera* cam, const rtw_params* p, void* ws, size_t ws_bytes,
                 uint8_t* d_rgb, float* d_mean, hipStream_t stream, rtw_timer timer, int mode,
                 uint32_t* tail_ran = nullptr, uint64_t seed_adv = 0, rtw_accum acc = nullptr) {
  if (!w || !cam) return rtw_fail(RTW_EINVAL, "world/camera is NULL");
  const int v = rtw_validate_params(p);
  if (v != RTW_OK) return v;
  if (p->precision != RTW_PRECISION_F64 || p->engine != RTW_ENGINE_MEGAKERNEL)
    return rtw_fail(RTW_UNSUPPORTED, "world renders run in f64 on the megakernel engine");
  if (w->has_moving && w->view.n_nodes && (cam->time0 < 0.0 || cam->time1 > 1.0))
    return rtw_fail(RTW_UNSUPPORTED, "BVH boxes of moving spheres cover shutter times [0, 1] only");
  const rtwp::WsLayout L = rtwp::ws_layout(p);
  int dev = 0;
  RtwPassMap map;  // a pass of a masked accumulator deals its active tiles only; with none it launches nothing
  bool launch = true;
  const int st0 = rtw_launch_begin(L, ws, ws_bytes, w->device, "world lives on device %d, current is %d", acc, timer,
                                   stream, &dev, &map, &launch);
  if (st0 != RTW_OK || !launch) {
    if (st0 == RTW_OK && tail_ran) *tail_ran = 0u;
    return st0;
  }
  auto* wsb = static_cast<unsigned char*>(ws);
  rtwk::WorldArgs a;
  std::memset(&a, 0, sizeof(a));
  rtw_fill_trace_args(a.t, cam, p, wsb, seed_adv);
  a.w = w->view;
  a.margin = bvh_margin(w, cam);
  a.counts = reinterpret_cast<unsigned long long*>(wsb + L.stats_off);
  const WorldLaunchCfg c = world_cfg(w, p, dev);
  // Tail dealing (default; development knob RTW_WORLD_TAIL=0: off) needs the
  // rings in the workspace (rtw_world_workspace_bytes); a workspace of only
  // rtw_workspace_bytes(params) renders without it — the same image, and
  // rtw_world_render_counts_ex reports which ran.
  const char* te = rtw_dev_knob("RTW_WORLD_TAIL");
  a.tail_deal = ((te && *te == '0') || ws_bytes < c.ring_off + c.ring_bytes) ? 0u : 1u;
  a.ring = a.tail_deal ? reinterpret_cast<double*>(wsb + c.ring_off) : nullptr;
  // per-lane traversal: pause a wave's walks once fewer than this many lanes
  // still walk (development knob RTW_WORLD_YIELD)
  const char* ye = rtw_dev_knob("RTW_WORLD_YIELD");
  a.lane_yield = (ye && *ye) ? (uint32_t)atoi(ye) : kLaneYield;
  if (tail_ran) *tail_ran = a.tail_deal;
  const size_t lds = c.lds;
  uint32_t grid = c.grid;
  map.apply(a.t);
  if (map.list)  // (the rings are sized for c.grid: a smaller grid uses their head)
    grid = std::max(1u, std::min(grid, (a.t.total_units + 255u) / 256u));
  const int oi = c.oi, fs = c.fs;
  if (timer && rtw_timer_mark(timer, stream, true) != RTW_OK) return RTW_EHIP;
  hipError_t e = rtwk::launch_world(a, grid, lds, stream, mode, oi, fs);
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "world kernel launch: %s", hipGetErrorString(e));
  if (timer && rtw_timer_mark(timer, stream, false) != RTW_OK) return RTW_EHIP;
  if (acc) return rtw_accum_pass_fold(acc, p, wsb, stream);  // a pass: the fold in the finalize launch's place
  if (d_rgb) return rtw_launch_finalize(p, wsb, d_rgb, d_mean, stream);
  return RTW_OK;
}

}  // namespace

extern "C" {

size_t rtw_world_workspace_bytes(rtw_world w, const rtw_params* p) {
  if (!w || rtw_validate_params(p) != RTW_OK) return 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev != w->device) {
    rtw_fail(RTW_EINVAL, "rtw_world_workspace_bytes: the world's device must be current");
    return 0;
  }
  const WorldLaunchCfg c = world_cfg(w, p, dev);
  return c.ring_off + c.ring_bytes;
}

int rtw_world_launch_info(rtw_world w, const rtw_params* p, uint32_t info_out[6]) {
  if (!w || !info_out) return rtw_fail(RTW_EINVAL, "world/info is NULL");
  const int v = rtw_validate_params(p);
  if (v != RTW_OK) return v;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev != w->device)
    return rtw_fail(RTW_EINVAL, "rtw_world_launch_info: the world's device must be current");
  const WorldLaunchCfg c = world_cfg(w, p, dev);
  info_out[0] = w->view.n_nodes == 0 ? RTW_WORLD_TRAVERSAL_LINEAR
                                     : ((c.fs & 16) ? RTW_WORLD_TRAVERSAL_LANE : RTW_WORLD_TRAVERSAL_UNION);
  info_out[1] = (uint32_t)c.fs;
  info_out[2] = (uint32_t)c.oi;
  info_out[3] = (uint32_t)c.bpc;
  info_out[4] = c.grid;
  info_out[5] = (uint32_t)c.lds;
  return RTW_OK;
}

int rtw_world_render_device(rtw_world w, const rtw_camera* cam, const rtw_params* p, void* ws, size_t ws_bytes,
                            uint8_t* d_rgb, float* d_mean, void* stream, rtw_timer timer) {
  if (!d_rgb) return rtw_fail(RTW_EINVAL, "d_rgb is NULL");
  return world_launch(w, cam, p, ws, ws_bytes, d_rgb, d_mean, static_cast<hipStream_t>(stream), timer, 0);
}

// The world's feature buffers (rtw_world.hip world_guides_kernel).
int rtw_world_guides_device(rtw_world w, const rtw_camera* cam, const rtw_params* p, rtw_guide* d_guides,
                            void* stream) {
  if (!w) return rtw_fail(RTW_EINVAL, "rtw_world_guides_device: world is NULL");
  rtwk::WorldGuideArgs a;
  const int st = rtw_guide_ray_fill(a.r, "rtw_world_guides_device", cam, p, d_guides);
  if (st != RTW_OK) return st;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return rtw_fail(RTW_ENODEV, "no HIP device");
  if (dev != w->device)
    return rtw_fail(RTW_EINVAL, "rtw_world_guides_device: world lives on device %d, current is %d", w->device, dev);
  a.w = w->view;
  const hipError_t e = rtwk::launch_world_guides(a, (w->feat & 64u) != 0u, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "guide kernel launch: %s", hipGetErrorString(e));
  return RTW_OK;
}

size_t rtw_accum_world_workspace_bytes(rtw_world w, const rtw_params* p, uint32_t pass_spp) {
  rtw_params pp;
  if (!w || !rtw_accum_size_params(p, pass_spp, &pp)) return 0;
  return rtw_world_workspace_bytes(w, &pp);
}

int rtw_accum_world_render_device(rtw_accum a, rtw_world w, const rtw_camera* cam, uint32_t pass_spp, void* ws,
                                  size_t ws_bytes, void* stream, rtw_timer timer) {
  if (!a || !w || !cam) return rtw_fail(RTW_EINVAL, "accumulator/world/camera is NULL");
  rtw_params pp;
  uint64_t adv = 0;
  const int st = rtw_accum_pass_begin(a, pass_spp, &pp, &adv);
  if (st != RTW_OK) return st;
  return world_launch(w, cam, &pp, ws, ws_bytes, nullptr, nullptr, static_cast<hipStream_t>(stream), timer, 0,
                      nullptr, adv, a);
}

int rtw_world_render_counts_ex(rtw_world w, const rtw_camera* cam, const rtw_params* p, void* ws, size_t ws_bytes,
                               uint64_t counts_out[8]) {
  if (!counts_out) return rtw_fail(RTW_EINVAL, "counts is NULL");
#ifdef RTW_MEASURE
  // RTW_WORLD_PHASE=1 (diagnostic build): a phase-stamp pass first; its wave-cycle
  // shares go to stderr (tools/world_bench.py --phase).
  const char* ph = rtw_dev_knob("RTW_WORLD_PHASE");
  if (ph && *ph == '1') {
    int st2 = world_launch(w, cam, p, ws, ws_bytes, nullptr, nullptr, nullptr, nullptr, 2);
    if (st2 != RTW_OK) return st2;
    unsigned long long q[5];
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(q, static_cast<unsigned char*>(ws) + rtwp::ws_layout(p).stats_off + 8 * 8, sizeof(q), hipMemcpyDeviceToHost) !=
            hipSuccess)
      return rtw_fail(RTW_EHIP, "world phase pass failed");
    double tot = 0;
    for (auto x : q) tot += (double)x;
    const char* nm[5] = {"tail/loop", "sample start + units", "node visits", "leaf primitives", "shading"};
    for (int i = 0; i < 5; ++i) fprintf(stderr, "[world phase] %-22s %6.2f %%\n", nm[i], 100.0 * (double)q[i] / tot);
  }
#endif
  uint32_t tail = 0;
  const int st = world_launch(w, cam, p, ws, ws_bytes, nullptr, nullptr, nullptr, nullptr, 1, &tail);
  if (st != RTW_OK) return st;
  if (hipDeviceSynchronize() != hipSuccess) return rtw_fail(RTW_EHIP, "world counts pass failed");
  unsigned long long c[7];
  if (hipMemcpy(c, static_cast<unsigned char*>(ws) + rtwp::ws_layout(p).stats_off, sizeof(c), hipMemcpyDeviceToHost) !=
      hipSuccess)
    return rtw_fail(RTW_EHIP, "counts copy failed");
  for (int i = 0; i < 5; ++i) counts_out[i] = c[i];  // samples, segments, node visits, primitive tests, wave iterations
  counts_out[5] = tail;
  counts_out[6] = c[5];  // per-lane traversal: interior-step wave iterations
  counts_out[7] = c[6];  // and leaf-test wave iterations
  return RTW_OK;
}

int rtw_world_render_counts(rtw_world w, const rtw_camera* cam, const rtw_params* p, void* ws, size_t ws_bytes,
                            uint64_t counts_out[4]) {
  if (!counts_out) return rtw_fail(RTW_EINVAL, "counts is NULL");
  uint64_t c[8];
  const int st = rtw_world_render_counts_ex(w, cam, p, ws, ws_bytes, c);
  if (st == RTW_OK)
    for (int i = 0; i < 4; ++i) counts_out[i] = c[i];
  return st;
}

}  // extern "C"

// ------------------------------------------------------------ ray queries --
// (rtw_hip.h "ray queries"; kernels: rtw_query.hip; checks, AUTO rule and launch geometry: rtw_query_plan.hpp)
namespace {

struct QueryCfg {
  uint32_t traversal;  // rtw_world_traversal: LANE, UNION or LINEAR
  int fs;              // the query kernel's feature set
};
QueryCfg query_cfg(const rtw_world_s* w, const rtw_query_opts* o) {
  // per lane: sphere worlds (image textures allowed) whose BVH fits the per-lane stack, as world_cfg
  const bool lane_ok = (w->feat & ~(2u | 64u)) == 0u && w->view.n_nodes > 0 && w->info[2] <= rtwk::kLaneStack &&
                       w->info[3] <= rtwk::kMaxLeafPrims && w->view.n_prims + 1u < (1u << rtwk::kTravPosBits);
  QueryCfg c;
  c.traversal = rtwq::traversal(o ? o->traversal : 0u, w->view.n_nodes, lane_ok);
  c.fs = c.traversal == RTW_WORLD_TRAVERSAL_LANE ? rtwk::world_feature_set(w->feat, true, w->packed) : (15 | (int)(w->feat & 64u));
  return c;
}
int query_bpc(int fs, bool occlusion) {  // resident workgroups per CU, asked once per kernel
  static std::mutex mu;
  static int cache[128][2] = {};
  std::lock_guard<std::mutex> lk(mu);
  int& e = cache[fs & 127][occlusion ? 1 : 0];
  if (e == 0) e = rtwk::query_blocks_per_cu(fs, occlusion);
  return e;
}

int mirror_bpc(int fs) {  // the mirror-point kernels' (rtw_specular.hip)
  static std::mutex mu;
  static int cache[64] = {};
  std::lock_guard<std::mutex> lk(mu);
  int& e = cache[fs & 63];
  if (e == 0) e = rtwk::mirror_blocks_per_cu(fs);
  return e;
}

// What a query kernel reads of the world (a: zeroed).
void query_args(const rtw_world_s* w, rtwk::WorldQueryArgs& a) {
  a.w = w->view;
  a.lane_yield = kLaneYield;
  a.seq_times = (w->has_moving && w->view.n_nodes) ? 1u : 0u;
  for (int k = 0; k < 3; ++k) {
    if (std::isfinite(w->bounds_lo[k])) a.reach = std::max(a.reach, std::fabs(w->bounds_lo[k]));
    if (std::isfinite(w->bounds_hi[k])) a.reach = std::max(a.reach, std::fabs(w->bounds_hi[k]));
  }
}

int world_query(const char* who, rtw_world w, const rtw_ray* d_rays, uint64_t n, const rtw_query_opts* opts,
                void* d_out, bool occlusion, hipStream_t stream) {
  std::string msg;
  const int st = rtwq::check_batch(who, w, d_rays, n, opts, d_out, occlusion ? 1u : 8u, msg);
  if (st != RTW_OK) return rtw_fail(st, "%s", msg.c_str());
  if (n == 0) return RTW_OK;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return rtw_fail(RTW_ENODEV, "no HIP device");
  if (dev != w->device) return rtw_fail(RTW_EINVAL, "%s: world lives on device %d, current is %d", who, w->device, dev);
  const QueryCfg c = query_cfg(w, opts);
  rtwk::WorldQueryArgs a;
  std::memset(&a, 0, sizeof(a));
  query_args(w, a);
  a.rays = reinterpret_cast<const double*>(d_rays);
  a.out = d_out;
  a.n = (uint32_t)n;
  const uint32_t grid = rtwq::grid(n, (uint32_t)rtw_device_cus(dev), (uint32_t)query_bpc(c.fs, occlusion));
  const hipError_t e = rtwk::launch_world_query(a, grid, c.fs, occlusion, stream);
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "%s: kernel launch: %s", who, hipGetErrorString(e));
  return RTW_OK;
}

}  // namespace

extern "C" {

int rtw_world_trace_device(rtw_world w, const rtw_ray* d_rays, uint64_t n, const rtw_query_opts* opts, rtw_hit* d_hits,
                           void* stream) {
  return world_query("rtw_world_trace_device", w, d_rays, n, opts, d_hits, false, static_cast<hipStream_t>(stream));
}

int rtw_world_occluded_device(rtw_world w, const rtw_ray* d_rays, uint64_t n, const rtw_query_opts* opts,
                              uint8_t* d_occluded, void* stream) {
  return world_query("rtw_world_occluded_device", w, d_rays, n, opts, d_occluded, true,
                     static_cast<hipStream_t>(stream));
}

int rtw_world_trace(rtw_world w, const rtw_ray* rays, uint64_t n, const rtw_query_opts* opts, rtw_hit* hits_out) {
  std::string msg;
  const int st = rtwq::check_batch("rtw_world_trace", w, rays, n, opts, hits_out, 8u, msg);
  if (st != RTW_OK) return rtw_fail(st, "%s", msg.c_str());
  if (n == 0) return RTW_OK;
  RtwQueryBuffers b;
  int rc = b.upload("rtw_world_trace", rays, n);
  if (rc == RTW_OK) rc = rtw_world_trace_device(w, b.d_rays, n, opts, b.d_hits, nullptr);
  if (rc == RTW_OK) rc = b.download("rtw_world_trace", hits_out, n);
  return rc;
}

int rtw_world_query_info(rtw_world w, const rtw_query_opts* opts, uint32_t info_out[4]) {
  if (!w || !info_out) return rtw_fail(RTW_EINVAL, "rtw_world_query_info: world/info is NULL");
  if (opts && (opts->traversal > RTW_WORLD_TRAVERSAL_LANE || opts->flags != 0))
    return rtw_fail(RTW_EINVAL, "rtw_world_query_info: opts.traversal %u / flags %u", opts->traversal, opts->flags);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev != w->device)
    return rtw_fail(RTW_EINVAL, "rtw_world_query_info: the world's device must be current");
  const QueryCfg c = query_cfg(w, opts);
  info_out[0] = c.traversal;
  info_out[1] = (uint32_t)c.fs;
  info_out[2] = rtwq::grid(RTW_QUERY_MAX_RAYS, (uint32_t)rtw_device_cus(dev), (uint32_t)query_bpc(c.fs, false));
  info_out[3] = (uint32_t)rtwk::query_lds_bytes(c.fs);
  return RTW_OK;
}

// (rtw_hip.h "mirror points"; kernels: rtw_specular.hip; the shared checks: rtw_specular_host.cpp)
int rtw_world_mirror_points_device(rtw_world w, const rtw_ray* d_rays, const rtw_hit* d_hits, uint64_t n,
                                   const rtw_camera* cam_prev, const double* d_a_prev, const double* d_xv_prev,
                                   const rtw_mirror_opts* opts, double* d_prev_p, rtw_hit* d_hits2, void* stream) {
  const char* who = "rtw_world_mirror_points_device";
  if (!w) return rtw_fail(RTW_EINVAL, "%s: world is NULL", who);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return rtw_fail(RTW_ENODEV, "no HIP device");
  if (dev != w->device) return rtw_fail(RTW_EINVAL, "%s: world lives on device %d, current is %d", who, w->device, dev);
  if (w->feat & 64u)  // rtw_world_walk.hpp kFeatTri
    return rtw_fail(RTW_UNSUPPORTED, "%s: the world holds triangles: mirror points are not built for them", who);
  if (n > RTW_QUERY_MAX_RAYS) return rtw_fail(RTW_EINVAL, "%s: n > 2^31", who);
  const rtw_mirror_opts dflt{};
  if (!opts) opts = &dflt;
  rtwk::WorldMirrorArgs a;
  std::memset(&a, 0, sizeof(a));
  if (n == 0) {
    if (!cam_prev || !rtwsp::resolve(opts->steps, opts->flags, a.steps))
      return rtw_fail(RTW_EINVAL, "%s: cam_prev is NULL or options out of range", who);
    return RTW_OK;
  }
  const int st = rtwsp::check_call(who, d_rays, d_hits, nullptr, n, cam_prev, d_a_prev, (size_t)72 * w->view.n_prims,
                                   d_xv_prev, (size_t)24 * RTW_MAX_XFORM_OPS * w->n_xforms, opts->steps, opts->flags,
                                   d_prev_p, d_hits2, a.steps);
  if (st != RTW_OK) return st;
  const QueryCfg c = query_cfg(w, nullptr);
  query_args(w, a.q);
  a.q.rays = reinterpret_cast<const double*>(d_rays);
  a.q.out = d_hits2;
  a.q.n = (uint32_t)n;
  a.hits = reinterpret_cast<const double*>(d_hits);
  a.a_prev = d_a_prev, a.xv_prev = d_xv_prev;
  a.prev_p = d_prev_p;
  for (int k = 0; k < 3; ++k) a.cam_o[k] = cam_prev->origin[k];
  const uint32_t grid = rtwq::grid(n, (uint32_t)rtw_device_cus(dev), (uint32_t)mirror_bpc(c.fs));
  const hipError_t e = rtwk::launch_world_mirror(a, grid, c.fs, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "%s: kernel launch: %s", who, hipGetErrorString(e));
  return RTW_OK;
}

int rtw_world_render(const rtw_camera* cam, const rtw_world_desc* desc, const rtw_params* p, uint8_t* rgb_out,
                     float* mean_out) {
  if (!cam || !desc || !rgb_out) return rtw_fail(RTW_EINVAL, "camera/desc/rgb_out is NULL");
  const int v = rtw_validate_params(p);
  if (v != RTW_OK) return v;
  RtwOneShot o;
  int st = o.enter(p);
  if (st != RTW_OK) return st;
  rtw_world w = nullptr;
  st = rtw_world_create(desc, 0, &w);
  if (st == RTW_OK) st = o.alloc("rtw_world_render", rtw_world_workspace_bytes(w, p), p, mean_out != nullptr);
  if (st == RTW_OK) st = world_launch(w, cam, p, o.ws, o.ws_bytes, o.d_rgb, o.d_mean, nullptr, nullptr, 0);
  if (st == RTW_OK && hipDeviceSynchronize() != hipSuccess) st = rtw_fail(RTW_EHIP, "world render failed on the device");
  if (st == RTW_OK) st = o.copy_back(rgb_out, mean_out);
  rtw_world_destroy(w);
  return st;
}

}  // extern "C"

int rtw_world_view(rtw_world w, const char* who, rtwk::WorldView* view, uint32_t* feat) {
  if (!w) return rtw_fail(RTW_EINVAL, "%s: world is NULL", who);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return rtw_fail(RTW_ENODEV, "no HIP device");
  if (dev != w->device) return rtw_fail(RTW_EINVAL, "%s: world lives on device %d, current is %d", who, w->device, dev);
  *view = w->view;
  if (feat) *feat = w->feat;
  return RTW_OK;
}

// ------------------------------------------------------ rtw_render --frames --
namespace rtw {

namespace {
// The numbers of frame k (rtw_orbit.hpp): the description's, turned by k * deg degrees.
void orbit_numbers(const rtw_world_desc& desc, uint32_t k, double deg, std::vector<rtw_prim>& prims,
                   std::vector<rtw_xform>& xforms) {
  const double phi = (double)k * deg * (3.14159265358979323846 / 180.0), sn = rtwl::sin(phi), cs = rtwl::cos(phi);
  for (uint32_t i = 0; i < desc.n_prims; ++i) {
    if (desc.prims[i].kind > RTW_PRIM_MOVING_SPHERE) continue;
    for (int e = 0; e < 2; ++e) {  // RotateY's forward map (hittable.zig:531-537) of both centres
      const double x = desc.prims[i].a[3 * e], z = desc.prims[i].a[3 * e + 2];
      prims[i].a[3 * e] = cs * x + sn * z, prims[i].a[3 * e + 2] = -sn * x + cs * z;
    }
  }
  for (uint32_t i = 0; i < desc.n_xforms; ++i)
    for (uint32_t c = 0; c < desc.xforms[i].n; ++c)
      if (desc.xforms[i].op[c] == RTW_XF_ROTATE_Y) {
        const double t = desc.xforms[i].v[c][2] + phi;
        xforms[i].v[c][0] = rtwl::sin(t), xforms[i].v[c][1] = rtwl::cos(t), xforms[i].v[c][2] = t;
      }
}

void ok(int st) {
  if (st != RTW_OK) throw Error(st, rtw_last_error());
}

// What a turntable holds on the device, released on every way out.
struct OrbitDev {
  rtw_world w = nullptr;
  std::vector<void*> bufs;
  ~OrbitDev() {
    for (void* b : bufs) (void)hipFree(b);
    rtw_world_destroy(w);
  }
  void* alloc(const char* who, size_t bytes) {
    void* b = nullptr;
    if (hipMalloc(&b, bytes ? bytes : 8) != hipSuccess) throw Error(RTW_ENOMEM, std::string(who) + ": device allocation failed");
    bufs.push_back(b);
    return b;
  }
};

// Frame k's numbers (k >= 1) given to the world: the update, and with rebuild_above >= 0 the tree's cost after
// it and a rebuild where that exceeds rebuild_above times the cost right after the creation or the last rebuild.
void orbit_apply(rtw_world w, const rtw_world_desc& desc, uint32_t k, double deg, double rebuild_above,
                 std::vector<rtw_prim>& prims, std::vector<rtw_xform>& xforms, double& built_cost) {
  orbit_numbers(desc, k, deg, prims, xforms);
  ok(rtw_world_update(w, prims.data(), desc.n_prims, xforms.data(), desc.n_xforms));
  if (rebuild_above < 0.0) return;
  double cost = 0.0;
  ok(rtw_world_bvh_cost(w, nullptr, &cost));
  if (cost > rebuild_above * built_cost) {
    ok(rtw_world_rebuild(w, prims.data(), desc.n_prims, xforms.data(), desc.n_xforms));
    ok(rtw_world_bvh_cost(w, nullptr, &built_cost));
    fprintf(stderr, "rebuild frame=%u cost_before=%.6g cost_after=%.6g\n", k, cost, built_cost);
  }
}
// A frame's feature buffers from its feature rays' first hits (rtw_hip.h "surface queries"), on the null
// stream, and their copy to the host.
struct GuidePass {
  rtw_ray* d_rays = nullptr;
  rtw_hit* d_hits = nullptr;
  rtw_guide* d_guides = nullptr;
  std::vector<rtw_guide> host;
  void alloc(OrbitDev& d, const char* who, size_t npix) {
    d_rays = static_cast<rtw_ray*>(d.alloc(who, npix * sizeof(rtw_ray)));
    d_hits = static_cast<rtw_hit*>(d.alloc(who, npix * sizeof(rtw_hit)));
    d_guides = static_cast<rtw_guide*>(d.alloc(who, npix * sizeof(rtw_guide)));
  }
  void run(rtw_world w, const rtw_camera& cam, uint32_t W, uint32_t H, const double bg[3]) {
    const size_t npix = (size_t)W * H;
    ok(rtw_pixel_rays_device(&cam, W, H, d_rays, nullptr));
    ok(rtw_world_trace_device(w, d_rays, npix, nullptr, d_hits, nullptr));
    ok(rtw_world_surface_device(w, d_hits, npix, bg, nullptr, d_guides, nullptr));
  }
  const std::vector<rtw_guide>& fetch(const rtw_guide* from, size_t npix) {
    host.resize(npix);
    if (hipMemcpy(host.data(), from, npix * sizeof(rtw_guide), hipMemcpyDeviceToHost) != hipSuccess)
      throw Error(RTW_EHIP, "the feature buffers failed on the device");
    return host;
  }
};
}  // namespace

std::vector<rtw_guide> frameGuides(const rtw_camera& cam, uint32_t W, uint32_t H, const double background[3],
                                   const rtw_world_desc& desc) {
  OrbitDev d;
  ok(rtw_world_create(&desc, 0, &d.w));
  GuidePass g;
  g.alloc(d, "frameGuides", (size_t)W * H);
  g.run(d.w, cam, W, H, background);
  return g.fetch(g.d_guides, (size_t)W * H);
}

void renderOrbit(const rtw_camera& cam, const rtw_params& p, const rtw_world_desc& desc, uint32_t frames, double deg,
                 const FrameFn& on_frame, double rebuild_above, const GuideFn& on_guides) {
  OrbitDev d;
  ok(rtw_world_create(&desc, RTW_WORLD_DYNAMIC, &d.w));
  const size_t wsb = rtw_world_workspace_bytes(d.w, &p);
  if (wsb == 0) throw Error(RTW_EINVAL, rtw_last_error());
  if (on_guides && (p.row_begin != 0 || p.row_stride != 1 || p.row_count != p.height))
    throw Error(RTW_UNSUPPORTED, "renderOrbit: the feature buffers need whole frames of contiguous rows");
  std::vector<uint8_t> rgb((size_t)p.width * p.row_count * 3);
  void* ws = d.alloc("renderOrbit", wsb);
  uint8_t* d_rgb = static_cast<uint8_t*>(d.alloc("renderOrbit", rgb.size()));
  GuidePass gp;
  if (on_guides) gp.alloc(d, "renderOrbit", (size_t)p.width * p.height);
  std::vector<rtw_prim> prims(desc.prims, desc.prims + desc.n_prims);
  std::vector<rtw_xform> xforms(desc.xforms, desc.xforms + desc.n_xforms);
  double built_cost = 0.0;  // the tree cost right after the creation or the last rebuild
  if (rebuild_above >= 0.0) ok(rtw_world_bvh_cost(d.w, nullptr, &built_cost));
  for (uint32_t k = 0; k < frames; ++k) {
    if (k) orbit_apply(d.w, desc, k, deg, rebuild_above, prims, xforms, built_cost);  // (frame 0: the description as it stands)
    ok(rtw_world_render_device(d.w, &cam, &p, ws, wsb, d_rgb, nullptr, nullptr, nullptr));
    if (hipMemcpy(rgb.data(), d_rgb, rgb.size(), hipMemcpyDeviceToHost) != hipSuccess)
      throw Error(RTW_EHIP, "renderOrbit: the render failed on the device");
    on_frame(k, rgb);
    if (on_guides) {
      gp.run(d.w, cam, p.width, p.height, p.background);
      on_guides(k, gp.fetch(gp.d_guides, (size_t)p.width * p.height));
    }
  }
}

// The frames of renderOrbit, each accumulated over the ones before it (rtw_hip.h "temporal accumulation").
void renderOrbitTemporal(const rtw_camera& cam, const rtw_params& p0, const rtw_world_desc& desc, uint32_t frames,
                         double deg, const FrameFn& on_frame, const TemporalRun& run, double rebuild_above,
                         const GuideFn& on_guides, const rtw_temporal_clamp* clamp, const rtw_mirror_opts* mirror) {
  const char* who = "renderOrbitTemporal";
  OrbitDev d;
  if (p0.row_begin != 0 || p0.row_stride != 1 || p0.row_count != p0.height)
    throw Error(RTW_UNSUPPORTED, "renderOrbitTemporal: the accumulation needs whole frames of contiguous rows");
  ok(rtw_world_create(&desc, RTW_WORLD_DYNAMIC, &d.w));
  rtw_params p = p0;
  const size_t wsb = rtw_world_workspace_bytes(d.w, &p);
  if (wsb == 0) throw Error(RTW_EINVAL, rtw_last_error());
  const uint32_t W = p.width, H = p.height;
  const size_t npix = (size_t)W * H, na = (size_t)9 * desc.n_prims, nxv = (size_t)3 * RTW_MAX_XFORM_OPS * desc.n_xforms;
  rtw_denoise_opts dn = run.dn;
  const size_t dnb = run.denoise ? rtw_denoise_workspace_bytes(W, H, &dn) : 0;
  if (run.denoise && dnb == 0) throw Error(RTW_EINVAL, rtw_last_error());
  void* ws = d.alloc(who, wsb);
  uint8_t* d_rgb = static_cast<uint8_t*>(d.alloc(who, npix * 3));
  float* d_mean = static_cast<float*>(d.alloc(who, npix * 12));
  float* d_acc = static_cast<float*>(d.alloc(who, npix * 12));
  float* d_var = static_cast<float*>(d.alloc(who, npix * 4));
  rtw_ray* d_rays = static_cast<rtw_ray*>(d.alloc(who, npix * sizeof(rtw_ray)));
  rtw_hit* d_hits = static_cast<rtw_hit*>(d.alloc(who, npix * sizeof(rtw_hit)));
  rtw_guide* d_guides = static_cast<rtw_guide*>(d.alloc(who, npix * sizeof(rtw_guide)));
  double* d_pp = static_cast<double*>(d.alloc(who, npix * 24));
  rtw_history* d_hist[2] = {static_cast<rtw_history*>(d.alloc(who, npix * sizeof(rtw_history))),
                            static_cast<rtw_history*>(d.alloc(who, npix * sizeof(rtw_history)))};
  double* d_a_prev = static_cast<double*>(d.alloc(who, na * 8));
  double* d_xv_prev = static_cast<double*>(d.alloc(who, nxv * 8));
  void* d_dn = run.denoise ? d.alloc(who, dnb) : nullptr;
  rtw_temporal_opts to{};
  to.max_history = run.max_history;
  std::vector<uint8_t> rgb(npix * 3);
  GuidePass guide_copy;  // (its host vector only: the guides are the loop's own)
  std::vector<float> acc;
  std::vector<rtw_prim> prims(desc.prims, desc.prims + desc.n_prims);
  std::vector<rtw_xform> xforms(desc.xforms, desc.xforms + desc.n_xforms);
  std::vector<double> a_prev(na), xv_prev(nxv);
  const bool moves = deg != 0.0;  // (a turn of 0 degrees: nothing moved, no previous points)
  const double time = cam.time0 + 0.5 * (cam.time1 - cam.time0);  // the feature ray's
  double built_cost = 0.0;
  if (rebuild_above >= 0.0) ok(rtw_world_bvh_cost(d.w, nullptr, &built_cost));
  for (uint32_t k = 0; k < frames; ++k) {
    if (k) {
      if (moves) {  // the previous frame's numbers stay on the device for the reprojection
        for (uint32_t i = 0; i < desc.n_prims; ++i) std::memcpy(&a_prev[(size_t)9 * i], prims[i].a, sizeof(prims[i].a));
        for (uint32_t i = 0; i < desc.n_xforms; ++i) std::memcpy(&xv_prev[(size_t)12 * i], xforms[i].v, sizeof(xforms[i].v));
        if ((na && hipMemcpy(d_a_prev, a_prev.data(), na * 8, hipMemcpyHostToDevice) != hipSuccess) ||
            (nxv && hipMemcpy(d_xv_prev, xv_prev.data(), nxv * 8, hipMemcpyHostToDevice) != hipSuccess))
          throw Error(RTW_EHIP, "renderOrbitTemporal: upload of the previous numbers failed");
      }
      orbit_apply(d.w, desc, k, deg, rebuild_above, prims, xforms, built_cost);
    }
    p.seed = p0.seed + k;  // equal seeds give equal noise, which no mean reduces
    ok(rtw_world_render_device(d.w, &cam, &p, ws, wsb, d_rgb, d_mean, nullptr, nullptr));
    ok(rtw_pixel_rays_device(&cam, W, H, d_rays, nullptr));
    ok(rtw_world_trace_device(d.w, d_rays, npix, nullptr, d_hits, nullptr));
    // the frame's guides from the hits it already has: rtw_world_guides_device's bytes
    ok(rtw_world_surface_device(d.w, d_hits, npix, p.background, nullptr, d_guides, nullptr));
    const bool reproject = k && moves;
    if (reproject && mirror)  // (the feature rays all carry `time`)
      ok(rtw_world_mirror_points_device(d.w, d_rays, d_hits, npix, &cam, na ? d_a_prev : nullptr,
                                        nxv ? d_xv_prev : nullptr, mirror, d_pp, nullptr, nullptr));
    else if (reproject)
      ok(rtw_world_prev_points_device(d.w, d_hits, npix, time, na ? d_a_prev : nullptr, nxv ? d_xv_prev : nullptr, d_pp,
                                      nullptr));
    if (clamp)
      ok(rtw_temporal_clamped_device(d_mean, d_guides, reproject ? d_pp : nullptr, &cam, &cam,
                                     k ? d_hist[(k + 1) & 1] : nullptr, W, H, &to, clamp, d_hist[k & 1], d_acc, d_var,
                                     nullptr));
    else
      ok(rtw_temporal_device(d_mean, d_guides, reproject ? d_pp : nullptr, &cam, &cam, k ? d_hist[(k + 1) & 1] : nullptr, W,
                             H, &to, d_hist[k & 1], d_acc, d_var, nullptr));
    if (run.denoise) {
      ok(rtw_denoise_device(d_acc, d_var, d_guides, W, H, &dn, d_dn, dnb, d_rgb, nullptr, nullptr));
      if (hipMemcpy(rgb.data(), d_rgb, rgb.size(), hipMemcpyDeviceToHost) != hipSuccess)
        throw Error(RTW_EHIP, "renderOrbitTemporal: the frame failed on the device");
    } else if (k == 0) {  // the first frame's accumulated mean is the render's own: so is its image
      if (hipMemcpy(rgb.data(), d_rgb, rgb.size(), hipMemcpyDeviceToHost) != hipSuccess)
        throw Error(RTW_EHIP, "renderOrbitTemporal: the frame failed on the device");
    } else {  // the accumulated mean, quantised as a render's
      acc.resize(npix * 3);
      if (hipMemcpy(acc.data(), d_acc, acc.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
        throw Error(RTW_EHIP, "renderOrbitTemporal: the frame failed on the device");
      for (size_t i = 0; i < acc.size(); ++i) rgb[i] = rtwd::quantise((double)acc[i]);
    }
    on_frame(k, rgb);
    if (on_guides) on_guides(k, guide_copy.fetch(d_guides, npix));
  }
}

}  // namespace rtw
