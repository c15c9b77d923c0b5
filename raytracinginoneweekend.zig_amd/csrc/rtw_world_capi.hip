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

#include "rtw_hip.h"
#include "rtw_capi_shared.hpp"
#include "rtw_internal.hpp"
#include "rtw_world_pack.hpp"

struct rtw_world_s {
  int device = 0;
  void* buf = nullptr;
  rtwk::WorldView view{};
  double bounds_lo[3] = {0, 0, 0}, bounds_hi[3] = {0, 0, 0};  // box of every primitive (+-inf when empty)
  bool has_moving = false;
  uint32_t feat = 0;  // features used (rtw_world.hip kFeat*): picks the kernel instantiation
  uint32_t info[4] = {0, 0, 0, 0};
  bool packed = false;  // the BVH carries the refs in its bounds' low bits (rtw_world_pack.cpp pack_refs)
};

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
  *out = w;
  return RTW_OK;
}

int rtw_world_destroy(rtw_world w) {
  if (!w) return RTW_OK;
  if (w->buf) (void)hipFree(w->buf);
  delete w;
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
  return (w->feat & (4u | 8u)) ? 3 : 4;  // rtw_world.hip kFeatXform | kFeatRect
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
  const uint32_t feat = p->world_features == RTW_WORLD_FEATURES_ALL ? 15u : w->feat;
  // AUTO: per lane on BVHs of >= kLaneNodes nodes (configs[4]'s globe: 5,802
  // nodes, +30 %); the union walk on small trees, where the lanes' paths
  // mostly coincide (scene 1's 23 nodes: the union 17 % faster).
  const bool lane_ok = w->view.n_nodes > 0 && w->info[2] <= rtwk::kLaneStack && w->info[3] <= rtwk::kMaxLeafPrims &&
                       w->view.n_prims + 1u < (1u << rtwk::kTravPosBits);
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
  static int bpc_cache[64][5] = {};
  static size_t bpc_lds[64][5] = {};
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
  const hipError_t e = rtwk::launch_world_guides(a, static_cast<hipStream_t>(stream));
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
  const bool lane_ok = (w->feat & ~2u) == 0u && w->view.n_nodes > 0 && w->info[2] <= rtwk::kLaneStack &&
                       w->info[3] <= rtwk::kMaxLeafPrims && w->view.n_prims + 1u < (1u << rtwk::kTravPosBits);
  QueryCfg c;
  c.traversal = rtwq::traversal(o ? o->traversal : 0u, w->view.n_nodes, lane_ok);
  c.fs = c.traversal == RTW_WORLD_TRAVERSAL_LANE ? rtwk::world_feature_set(w->feat, true, w->packed) : 15;
  return c;
}
int query_bpc(int fs, bool occlusion) {  // resident workgroups per CU, asked once per kernel
  static std::mutex mu;
  static int cache[64][2] = {};
  std::lock_guard<std::mutex> lk(mu);
  int& e = cache[fs & 63][occlusion ? 1 : 0];
  if (e == 0) e = rtwk::query_blocks_per_cu(fs, occlusion);
  return e;
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
  a.w = w->view;
  a.rays = reinterpret_cast<const double*>(d_rays);
  a.out = d_out;
  a.n = (uint32_t)n;
  a.lane_yield = kLaneYield;
  a.seq_times = (w->has_moving && w->view.n_nodes) ? 1u : 0u;
  for (int k = 0; k < 3; ++k) {
    if (std::isfinite(w->bounds_lo[k])) a.reach = std::max(a.reach, std::fabs(w->bounds_lo[k]));
    if (std::isfinite(w->bounds_hi[k])) a.reach = std::max(a.reach, std::fabs(w->bounds_hi[k]));
  }
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
