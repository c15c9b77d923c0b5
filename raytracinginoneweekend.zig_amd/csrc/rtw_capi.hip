// rtw_capi.hip — the C ABI (include/rtw_hip.h) of the cover-scene engines:
// error state, device info, scene upload, the launches of a render, the
// render and statistics entries, timers.  Replaces the render loop of
// src/main.zig:378-402.  No exception and no C++ type crosses the ABI.
// (Validation, sizes and layouts: rtw_plan.cpp; the wavefront engine's driver:
// rtw_wavefront_host.hip; the accumulator: rtw_accum_capi.hip.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "rtw_hip.h"
#include "rtw_capi_shared.hpp"
#include "rtw_claim.hpp"
#include "rtw_internal.hpp"
#include "rtw_math.hpp"
#include "rtw_scene_pack.hpp"

namespace {

thread_local std::string g_err;

}  // namespace

int rtw_fail(int status, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return status;
}

namespace {

// Development knobs (tools/, A/B measurement) are read from the environment
// only in the -DRTW_MEASURE build; the product library's behaviour depends on
// its arguments alone (engine configuration: rtw_params, ABI v4).
const char* dev_knob(const char* name) {
#ifdef RTW_MEASURE
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

uint64_t splitmix_first(uint64_t seed) {  // SplitMix64.init(seed).next()
  uint64_t z = seed + 0x9e3779b97f4a7c15ULL;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

constexpr int kBpcTail = 16;
struct DevInfo {
  int cus = 0;
  // (precision, masked) -> (lds, blocks per CU); precision + kBpcTail: the same with the tail blocks
  std::map<std::pair<int, bool>, std::pair<size_t, int>> bpc;
};
std::mutex g_dev_mu;
std::map<int, DevInfo> g_dev;

int device_cus(int dev) {
  std::lock_guard<std::mutex> lk(g_dev_mu);
  auto& d = g_dev[dev];
  if (d.cus == 0) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    d.cus = v;
  }
  return d.cus;
}
int blocks_per_cu(int dev, int prec, size_t lds, bool masked, bool tail = false) {
  std::lock_guard<std::mutex> lk(g_dev_mu);
  auto& d = g_dev[dev];
  auto& e = d.bpc[{prec + (tail ? kBpcTail : 0), masked}];
  if (e.second == 0 || e.first != lds) e = {lds, rtwk::trace_blocks_per_cu(prec, lds, masked)};
  return e.second;
}

}  // namespace

struct rtw_scene_s {
  int device = 0;
  uint32_t n = 0, nm = 0, ng = 0;
  uint32_t n_static = 0, n_moving = 0, n_wide = 0;
  void* buf = nullptr;  // one allocation holding every table
  std::vector<std::pair<double, double>> groups;  // moving-sphere time groups (t0, t1)
  float cull_cmax_cl = 0.0f;                       // Cmax over members and cluster centres
  rtwk::SceneView<double> v64{};
  rtwk::SceneView<float> v32{};
};

// (rtw_timer_s, rtw_accum_s: rtw_capi_shared.hpp)
struct rtw_sclk_probe_s {
  double* d = nullptr;  // [0] = MHz (device)
  hipStream_t s = nullptr;
};

namespace {
// One wave: spin (s_sleep between reads) until `ticks` of the constant-rate
// s_memrealtime counter passed; the SIMD clock = delta(s_memtime) /
// delta(s_memrealtime) x the counter's rate (hipDeviceAttributeWallClockRate,
// 100 MHz on MI355X; MI355X_MICROARCH.md: in-kernel clock).  Lane 0 writes it.
__global__ void __launch_bounds__(64) sclk_probe_kernel(unsigned long long ticks, double rt_mhz, double* out) {
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  unsigned long long r = r0;
  while (r - r0 < ticks) {
    __builtin_amdgcn_s_sleep(63);
    r = __builtin_amdgcn_s_memrealtime();
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) out[0] = (double)(t1 - t0) / (double)(r - r0) * rt_mhz;
}

// The view of precision R over a packed scene uploaded at `b`.  The clustered
// pretest is f64 only: there the view carries cmax_all (cluster centres
// included) when the scene's clusters are usable; cluster_on is then narrowed
// per render (launch_all).
template <typename R>
rtwk::SceneView<R> scene_view(const rtwp::ScenePack& k, const unsigned char* b) {
  using namespace rtwp;
  constexpr bool f64 = sizeof(R) == 8;
  auto P = [&](SceneTable t64, SceneTable t32) { return reinterpret_cast<const R*>(b + k.off[f64 ? t64 : t32]); };
  auto D = [&](SceneTable t) { return reinterpret_cast<const double*>(b + k.off[t]); };
  auto F = [&](SceneTable t) { return reinterpret_cast<const float*>(b + k.off[t]); };
  auto U = [&](SceneTable t) { return reinterpret_cast<const uint32_t*>(b + k.off[t]); };
  const uint32_t cl_ok = f64 ? k.cluster_ok : 0u;
  return {P(kSph64, kSph32), P(kRad64, kRad32), U(kMeta), P(kMat64, kMat32), U(kKind), P(kTg64, kTg32), D(kSph64),
          D(kTg64), U(kPerm), F(kCull), U(kCullTg), F(kTg32), k.n, k.nm, k.ng, k.g_end[0], k.g_end[1], k.g_end[2],
          k.nn, k.nn_pad, k.n_sn, k.cull_on, cl_ok ? k.cmax_all : k.cmax, k.rho, F(kCcull), U(kCcullTg), F(kCclus),
          U(kCpos), U(kCvalid), k.n_clusters, cl_ok, k.rho_c};
}
}  // namespace

extern "C" {

int rtw_abi_version(void) { return RTW_ABI_VERSION; }

const char* rtw_last_error(void) { return g_err.c_str(); }

int rtw_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int rtw_scene_create(const rtw_sphere* spheres, uint32_t n, const rtw_material* mats, uint32_t nm,
                     rtw_scene* out) {
  if (!out) return rtw_fail(RTW_EINVAL, "rtw_scene_create: out is NULL");
  *out = nullptr;
  rtwp::ScenePack k;
  std::string msg;
  const int st = rtwp::pack_scene(spheres, n, mats, nm, k, msg);
  if (st != RTW_OK) return rtw_fail(st, "%s", msg.c_str());
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  const size_t total = k.blob.size();
  void* d = nullptr;
  if (hipMalloc(&d, total) != hipSuccess) return rtw_fail(RTW_ENOMEM, "rtw_scene_create: hipMalloc(%zu)", total);
  if (hipMemcpy(d, k.blob.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return rtw_fail(RTW_EHIP, "rtw_scene_create: hipMemcpy failed");
  }
  auto* sc = new rtw_scene_s;
  sc->device = dev;
  sc->n = k.n;
  sc->nm = k.nm;
  sc->ng = k.ng;
  sc->n_moving = k.n_moving;
  sc->n_static = k.n_static;
  sc->n_wide = k.n_wide;
  sc->buf = d;
  sc->v64 = scene_view<double>(k, static_cast<unsigned char*>(d));
  sc->v32 = scene_view<float>(k, static_cast<unsigned char*>(d));
  sc->cull_cmax_cl = k.cmax_all;
  sc->groups = std::move(k.groups);
  *out = sc;
  return RTW_OK;
}

int rtw_scene_destroy(rtw_scene sc) {
  if (!sc) return RTW_OK;
  if (sc->buf) (void)hipFree(sc->buf);
  delete sc;
  return RTW_OK;
}

}  // extern "C"

int rtw_validate_params(const rtw_params* p) {
  std::string msg;
  const int st = rtwp::validate_params(p, msg);
  return st == RTW_OK ? st : rtw_fail(st, "%s", msg.c_str());
}

namespace {

using rtwp::WsLayout;

// Unit dealing order (rtw_device.hpp dealt_unit): the development knob
// RTW_UNIT_ORDER=fwd|rev overrides the engine's default (-DRTW_MEASURE only).
uint32_t unit_order(uint32_t dflt) {
  const char* uo = dev_knob("RTW_UNIT_ORDER");
  if (uo && std::strcmp(uo, "fwd") == 0) return 0u;
  if (uo && std::strcmp(uo, "rev") == 0) return 1u;
  return dflt;
}
constexpr uint32_t kWorldUnitOrder = 1u;

template <typename R>
void fill_args(rtwk::TraceArgs<R>& a, const rtwk::SceneView<R>& v, const rtw_camera* cam, const rtw_params* p,
               unsigned char* ws, const WsLayout& L, uint64_t seed_adv) {
  std::memset(&a, 0, sizeof(a));
  a.sc = v;
  for (int k = 0; k < 3; ++k) {
    a.origin[k] = (R)cam->origin[k];
    a.horizontal[k] = (R)cam->horizontal[k];
    a.vertical[k] = (R)cam->vertical[k];
    a.llc[k] = (R)cam->lower_left_corner[k];
    a.cu[k] = (R)cam->u[k];
    a.cv[k] = (R)cam->v[k];
    a.bg[k] = (R)p->background[k];
  }
  a.lens_radius = (R)cam->lens_radius;
  a.time0 = (R)cam->time0;
  a.time1 = (R)cam->time1;
  a.tmin = (R)0.001;  // rayColor's t_min (main.zig:109)
  a.inv_w1 = (R)1 / ((R)p->width - (R)1);
  a.inv_h1 = (R)1 / ((R)p->height - (R)1);
  // Prefilter bound: root2 <= 2u(1+u)^2 * hb/a < tmin
  // whenever hb < pre_k * a, u = unit roundoff of R.
  const double u = sizeof(R) == 8 ? 0x1p-53 : 0x1p-24;
  a.pre_k = (R)((double)a.tmin / (2.5 * u));
  a.W = p->width;
  a.H = p->height;
  a.spp = p->spp;
  a.max_depth = p->max_depth;
  a.chunk = rtwp::eff_chunk(p);
  a.n_chunks = rtwp::n_chunks(p);
  a.row_begin = p->row_begin;
  a.row_stride = p->row_stride;
  a.row_count = p->row_count;
  a.tiles_x = rtwp::tiles_x(p);
  a.total_units = (uint32_t)rtwp::total_units(p);
  const rtwm::UDivMagic mu = rtwm::udiv_magic((uint32_t)rtwp::tile_units(1, a.n_chunks)), mt = rtwm::udiv_magic(a.tiles_x);
  a.upt_m = mu.m, a.upt_sh = mu.sh, a.tx_m = mt.m, a.tx_sh = mt.sh;
  // seed_adv: 0 for a frame; an accumulator pass starts at sample s0 of its
  // pixels' streams, s0 * (gamma << 16) further on (accum_pass_begin).
  a.seed_base = splitmix_first(p->seed) + seed_adv;
  // Unit dealing order (rtw_device.hpp dealt_unit): image order, top rows
  // first, for the cover-scene engines, last-first for the world kernel
  // (rtw_fill_trace_args), each the faster in the in-process A/Bs
  // (profiles/r03/unit_order_ab.txt); RTW_UNIT_ORDER=fwd|rev overrides.
  a.unit_order = unit_order(0u);
  a.empty_on = 0u;  // (launch_engine)
  a.partial = reinterpret_cast<double*>(ws + L.partial_off);
  a.counter = reinterpret_cast<uint32_t*>(ws + L.counter_off);
  a.stats = reinterpret_cast<unsigned long long*>(ws + L.stats_off);
}

// n_clusters: clusters whose slot -> position table (cpos) is staged, 0 unless
// the launched kernel runs the clustered pretest (f64 and clusters_usable):
// other paths neither read nor stage it.
size_t lds_bytes(const rtw_scene_s* sc, int prec, uint32_t n_clusters) {
  const size_t r = prec == 1 ? 4 : 8;
  return rtwk::kCoopLdsBytes + r * (8 * ((size_t)sc->n + 1) + (size_t)sc->n + 8 * (size_t)sc->nm + 4 * (size_t)sc->ng) +
         4 * ((size_t)sc->n + 1 + sc->nm + sc->n + rtwk::kClusterSlots * (size_t)n_clusters) + 16;
}

// The clustered pretest's bounding spheres hold each moving member over its
// time group's [t0, t1]: usable only when the camera's shutter lies inside
// every group's range (else the members' centres leave the bounds).
uint32_t clusters_usable(const rtw_scene_s* sc, const rtw_camera* cam) {
  if (!sc->v64.cluster_on) return 0u;
  for (const auto& g : sc->groups)
    if (!(cam->time0 >= g.first && cam->time1 <= g.second)) return 0u;
  return 1u;
}

// The launches of a render in precision R: its args, with a masked pass's map and the clusters narrowed (cl_on:
// the clustered pretest runs; f32 has none, its view's cluster_on is 0 already), then the wavefront engine's
// driver, or the trace launch on min(grid_cap, the units' workgroups) workgroups.
template <typename R>
int launch_engine(const rtwk::SceneView<R>& view, const rtw_camera* cam, const rtw_params* p, unsigned char* ws,
                  const WsLayout& L, uint64_t seed_adv, const RtwPassMap& map, uint32_t cl_on, int dev, size_t lds,
                  uint32_t grid_cap, hipStream_t stream, int mode, bool masked, size_t tail_lds) {
  rtwk::TraceArgs<R> a;
  fill_args(a, view, cam, p, ws, L, seed_adv);
  map.apply(a);
  a.sc.cluster_on = cl_on;
  if (!cl_on) a.sc.n_clusters = 0u;  // nothing to stage (lds_bytes)
  // The primary-first loop: the megakernel's f64 frame kernel with the clusters on and every clustered slot in
  // one 64-slot block (a lane's tile mask is two words); else the kernel runs the rotated loop.
  a.primary_on = (p->engine == RTW_ENGINE_MEGAKERNEL && rtwk::trace_primary_first((int)p->precision, masked) &&
                  cl_on && a.sc.n_clusters * rtwk::kClusterSlots <= 64u)
                     ? 1u
                     : 0u;
  // Its tail dealing, where launch_all found room for the tail blocks (tail_lds, after `lds`).
  a.tail_on = (a.primary_on && tail_lds) ? 1u : 0u;
  // Its batches of tiles that no camera ray can hit a sphere from are finished without tracing: the beam pass
  // answers for the wide spheres too, on the lanes after the slots, where they fit; at max_depth 0 a sample
  // adds nothing, not the background.  (RTW_TRACE_EMPTY=0, -DRTW_MEASURE only: off, for the A/B.)
  const uint32_t n_wide = a.sc.g_static_wide + (a.sc.g_moving_wide - a.sc.g_static);
  a.empty_on = (a.primary_on && a.max_depth >= 1u && a.sc.n_clusters * rtwk::kClusterSlots + n_wide <= 64u) ? 1u : 0u;
  if (const char* ek = dev_knob("RTW_TRACE_EMPTY"); ek && ek[0] == '0') a.empty_on = 0u;
  if (a.tail_on) lds += tail_lds;
  if (p->engine == RTW_ENGINE_WAVEFRONT) {
    if (mode == 2) return rtw_fail(RTW_UNSUPPORTED, "phase profile runs on the megakernel engine");
    return rtw_run_wavefront<R>(a, p, ws, L, dev, lds, stream, mode == 1);
  }
  const uint32_t grid = std::max(1u, std::min(grid_cap, (a.total_units + 255) / 256));
  // Its guided claims (rtw_claim.hpp): several batches per atomic in a run of proven-empty batches while the
  // queue is long, from the waves of this grid.  Only in a launch that can make such a claim: batches are
  // proven empty (empty_on) and the queue is at least 2 x claim_waves batches long, so that the guided K is 2
  // or more at its head; in any other launch every claim would be one batch, and the reserve's bookkeeping
  // cost a 20-sample pass of the cover frame 0.9 % (profiles/r19/README.md).
  // (RTW_TRACE_CLAIM=1, -DRTW_MEASURE only: claims of one batch and no proof reuse, for the A/B.)
  const uint32_t claim_waves = rtwc::kClaimDiv * grid * (uint32_t)(rtwk::kTraceBlock / 64);
  a.claim_waves = (a.empty_on && a.total_units / rtwk::kBatch >= 2u * claim_waves) ? claim_waves : 0u;
  if (const char* ck = dev_knob("RTW_TRACE_CLAIM"); ck && ck[0] == '1') a.claim_waves = 0u;
  hipError_t e;
  if constexpr (sizeof(R) == 8)
    e = rtwk::launch_trace_f64(a, grid, lds, stream, mode, masked);
  else
    e = rtwk::launch_trace_f32(a, grid, lds, stream, mode, masked);
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "trace kernel launch: %s", hipGetErrorString(e));
  return RTW_OK;
}

// acc: the render is a pass of this accumulator (p->spp = the pass's samples,
// seed_adv = its offset into the pixels' sample streams): the fold takes the
// place of the finalize launch, ordered as that launch is — on `stream`,
// which the wavefront engine's queue sets have joined by then.
int launch_all(rtw_scene sc, const rtw_camera* cam, const rtw_params* p, void* workspace, size_t ws_bytes,
               uint8_t* d_rgb, float* d_mean, hipStream_t stream, rtw_timer timer, int mode,
               uint64_t seed_adv = 0, rtw_accum acc = nullptr) {
  const WsLayout L = rtwp::ws_layout(p);
  int dev = 0;
  RtwPassMap map;
  bool launch = true;
  const int st0 = rtw_launch_begin(L, workspace, ws_bytes, sc->device,
                                   "scene lives on device %d but the current device is %d", acc, timer, stream, &dev,
                                   &map, &launch);
  if (st0 != RTW_OK || !launch) return st0;
  auto* ws = static_cast<unsigned char*>(workspace);
  const bool masked = map.list && p->engine == RTW_ENGINE_MEGAKERNEL;  // the megakernel's masked configuration
  // The clustered pretest runs only in f64 (both engines), and only when the
  // shutter lies in every time group.
  const uint32_t cl_on = p->precision == RTW_PRECISION_F64 ? clusters_usable(sc, cam) : 0u;
  size_t lds = lds_bytes(sc, (int)p->precision, cl_on ? sc->v64.n_clusters : 0u);
  if (p->engine == RTW_ENGINE_MEGAKERNEL) lds += rtwk::trace_home_lds_bytes((int)p->precision, masked);
  if (lds > 64 * 1024) return rtw_fail(RTW_UNSUPPORTED, "scene tables need %zu B of LDS", lds);
  const int bpc = blocks_per_cu(dev, (int)p->precision, lds, masked);
  const uint32_t grid_cap = (uint32_t)(device_cus(dev) * bpc);
  // The tail blocks of the primary-first loop (TraceArgs::tail_on) join the launch only where they cost no
  // resident workgroup: a scene with large tables keeps the loop without the tail dealing.
  // (RTW_TRACE_TAIL=0, -DRTW_MEASURE only: off, for the A/B.)
  size_t tail_lds = p->engine == RTW_ENGINE_MEGAKERNEL ? rtwk::trace_tail_lds_bytes((int)p->precision, masked) : 0;
  if (const char* tk = dev_knob("RTW_TRACE_TAIL"); tk && tk[0] == '0') tail_lds = 0;
  if (tail_lds && (lds + tail_lds > 64 * 1024 || blocks_per_cu(dev, (int)p->precision, lds + tail_lds, masked, true) != bpc))
    tail_lds = 0;
  if (timer) HIP_TRY(hipEventRecord(timer->start, stream));
  const int st = p->precision == RTW_PRECISION_F32
                     ? launch_engine(sc->v32, cam, p, ws, L, seed_adv, map, cl_on, dev, lds, grid_cap, stream, mode,
                                     masked, tail_lds)
                     : launch_engine(sc->v64, cam, p, ws, L, seed_adv, map, cl_on, dev, lds, grid_cap, stream, mode,
                                     masked, tail_lds);
  if (st != RTW_OK) return st;
  if (timer) {
    HIP_TRY(hipEventRecord(timer->stop, stream));
    timer->recorded = true;
  }
  if (acc) return rtw_accum_pass_fold(acc, p, ws, stream);
  if (d_rgb) return rtw_launch_finalize(p, ws, d_rgb, d_mean, stream);
  return RTW_OK;
}
}  // namespace

extern "C" {

size_t rtw_workspace_bytes(const rtw_params* p) {
  if (rtw_validate_params(p) != RTW_OK) return 0;
  return rtwp::ws_layout(p).total;
}

int rtw_timer_create(rtw_timer* out) {
  if (!out) return rtw_fail(RTW_EINVAL, "timer out is NULL");
  auto* t = new rtw_timer_s;
  if (hipEventCreate(&t->start) != hipSuccess || hipEventCreate(&t->stop) != hipSuccess) {
    delete t;
    return rtw_fail(RTW_EHIP, "hipEventCreate failed");
  }
  *out = t;
  return RTW_OK;
}
int rtw_timer_destroy(rtw_timer t) {
  if (!t) return RTW_OK;
  (void)hipEventDestroy(t->start);
  (void)hipEventDestroy(t->stop);
  delete t;
  return RTW_OK;
}
int rtw_sclk_probe_begin(void* stream, double wall_ms, rtw_sclk_probe* out) {
  if (!out) return rtw_fail(RTW_EINVAL, "probe out is NULL");
  *out = nullptr;
  if (!(wall_ms > 0.0 && wall_ms < 600e3)) return rtw_fail(RTW_EINVAL, "probe window %g ms outside (0, 600 s)", wall_ms);
  // the s_memrealtime rate of the current device (kHz), not an assumed 100 MHz
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0)
    return rtw_fail(RTW_EHIP, "probe: wall-clock rate of device %d unavailable", dev);
  auto* p = new rtw_sclk_probe_s;
  p->s = static_cast<hipStream_t>(stream);
  if (hipMalloc(reinterpret_cast<void**>(&p->d), sizeof(double)) != hipSuccess) {
    delete p;
    return rtw_fail(RTW_ENOMEM, "probe: hipMalloc failed");
  }
  hipLaunchKernelGGL(sclk_probe_kernel, dim3(1), dim3(64), 0, p->s, (unsigned long long)(wall_ms * khz),
                     (double)khz * 1e-3, p->d);
  if (hipGetLastError() != hipSuccess) {
    (void)hipFree(p->d);
    delete p;
    return rtw_fail(RTW_EHIP, "probe kernel launch failed");
  }
  *out = p;
  return RTW_OK;
}
int rtw_sclk_probe_end(rtw_sclk_probe p, double* mhz) {
  if (!p || !mhz) return rtw_fail(RTW_EINVAL, "probe/mhz is NULL");
  int st = RTW_OK;
  if (hipStreamSynchronize(p->s) != hipSuccess || hipMemcpy(mhz, p->d, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    st = rtw_fail(RTW_EHIP, "probe read failed");
  (void)hipFree(p->d);
  delete p;
  return st;
}

int rtw_timer_elapsed_ms(rtw_timer t, float* ms) {
  if (!t || !ms) return rtw_fail(RTW_EINVAL, "timer/ms is NULL");
  if (!t->recorded) return rtw_fail(RTW_EINVAL, "timer was never recorded");
  HIP_TRY(hipEventSynchronize(t->stop));
  HIP_TRY(hipEventElapsedTime(ms, t->start, t->stop));
  return RTW_OK;
}

int rtw_render_device(rtw_scene sc, const rtw_camera* cam, const rtw_params* p, void* workspace,
                      size_t ws_bytes, uint8_t* d_rgb, float* d_mean, void* stream, rtw_timer timer) {
  if (!sc || !cam) return rtw_fail(RTW_EINVAL, "scene/camera is NULL");
  if (!d_rgb) return rtw_fail(RTW_EINVAL, "d_rgb is NULL");
  const int v = rtw_validate_params(p);
  if (v != RTW_OK) return v;
  return launch_all(sc, cam, p, workspace, ws_bytes, d_rgb, d_mean, static_cast<hipStream_t>(stream), timer, 0);
}

// A pass of an accumulator (rtw_accum_capi.hip) over a scene.
int rtw_accum_render_device(rtw_accum a, rtw_scene sc, const rtw_camera* cam, uint32_t pass_spp, void* workspace,
                            size_t ws_bytes, void* stream, rtw_timer timer) {
  if (!a || !sc || !cam) return rtw_fail(RTW_EINVAL, "accumulator/scene/camera is NULL");
  rtw_params pp;
  uint64_t adv = 0;
  const int st = rtw_accum_pass_begin(a, pass_spp, &pp, &adv);
  if (st != RTW_OK) return st;
  return launch_all(sc, cam, &pp, workspace, ws_bytes, nullptr, nullptr, static_cast<hipStream_t>(stream), timer, 0,
                    adv, a);
}

// The scene's feature buffers (rtw_guides.hip).
int rtw_scene_guides_device(rtw_scene sc, const rtw_camera* cam, const rtw_params* p, rtw_guide* d_guides,
                            void* stream) {
  if (!sc) return rtw_fail(RTW_EINVAL, "rtw_scene_guides_device: scene is NULL");
  rtwk::SceneGuideArgs a;
  const int st = rtw_guide_ray_fill(a.r, "rtw_scene_guides_device", cam, p, d_guides);
  if (st != RTW_OK) return st;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != sc->device)
    return rtw_fail(RTW_EINVAL, "rtw_scene_guides_device: scene lives on device %d, current is %d", sc->device, dev);
  a.sc = sc->v64;
  const hipError_t e = rtwk::launch_scene_guides(a, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "guide kernel launch: %s", hipGetErrorString(e));
  return RTW_OK;
}

}  // extern "C"

int rtw_scene_view(rtw_scene sc, const char* who, rtwk::SceneView<double>* view) {
  if (!sc) return rtw_fail(RTW_EINVAL, "%s: scene is NULL", who);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return rtw_fail(RTW_ENODEV, "no HIP device");
  if (dev != sc->device) return rtw_fail(RTW_EINVAL, "%s: scene lives on device %d, current is %d", who, sc->device, dev);
  *view = sc->v64;
  return RTW_OK;
}

extern "C" {

// Ray queries over a scene (rtw_hip.h "ray queries"; rtw_query.hip scene_query_kernel).
static int scene_query(const char* who, rtw_scene sc, const rtw_ray* d_rays, uint64_t n, void* d_out, bool occlusion,
                       void* stream) {
  std::string msg;
  const int st = rtwq::check_batch(who, sc, d_rays, n, nullptr, d_out, occlusion ? 1u : 8u, msg);
  if (st != RTW_OK) return rtw_fail(st, "%s", msg.c_str());
  if (n == 0) return RTW_OK;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != sc->device) return rtw_fail(RTW_EINVAL, "%s: scene lives on device %d, current is %d", who, sc->device, dev);
  rtwk::SceneQueryArgs a;
  a.sc = sc->v64;
  a.rays = reinterpret_cast<const double*>(d_rays);
  a.out = d_out;
  a.n = (uint32_t)n;
  const uint32_t grid = rtwq::grid(n, (uint32_t)device_cus(dev), 8u);
  const hipError_t e = rtwk::launch_scene_query(a, grid, occlusion, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "%s: kernel launch: %s", who, hipGetErrorString(e));
  return RTW_OK;
}
int rtw_scene_trace_device(rtw_scene sc, const rtw_ray* d_rays, uint64_t n, rtw_hit* d_hits, void* stream) {
  return scene_query("rtw_scene_trace_device", sc, d_rays, n, d_hits, false, stream);
}
int rtw_scene_occluded_device(rtw_scene sc, const rtw_ray* d_rays, uint64_t n, uint8_t* d_occluded, void* stream) {
  return scene_query("rtw_scene_occluded_device", sc, d_rays, n, d_occluded, true, stream);
}
int rtw_scene_trace(rtw_scene sc, const rtw_ray* rays, uint64_t n, rtw_hit* hits_out) {
  std::string msg;
  const int st = rtwq::check_batch("rtw_scene_trace", sc, rays, n, nullptr, hits_out, 8u, msg);
  if (st != RTW_OK) return rtw_fail(st, "%s", msg.c_str());
  if (n == 0) return RTW_OK;
  RtwQueryBuffers b;
  int rc = b.upload("rtw_scene_trace", rays, n);
  if (rc == RTW_OK) rc = rtw_scene_trace_device(sc, b.d_rays, n, b.d_hits, nullptr);
  if (rc == RTW_OK) rc = b.download("rtw_scene_trace", hits_out, n);
  return rc;
}

// The statistics pass: one render in counting mode, the kernels' 32 statistics
// words copied back (rtw_hip.h RTW_STAT_*; words 16.. are the diagnostic
// build's phase stamps).
static int stats_pass(rtw_scene sc, const rtw_camera* cam, const rtw_params* p, void* workspace, size_t ws_bytes,
               unsigned long long (&st)[32]) {
  if (!sc || !cam) return rtw_fail(RTW_EINVAL, "scene/camera is NULL");
  const int v = rtw_validate_params(p);
  if (v != RTW_OK) return v;
  // RTW_PHASE_PROFILE=1: diagnostic build with per-phase s_memtime stamps.
  const char* prof = dev_knob("RTW_PHASE_PROFILE");
  const int mode = (prof && prof[0] == '1') ? 2 : 1;
#ifndef RTW_MEASURE
  if (mode == 2) return rtw_fail(RTW_UNSUPPORTED, "RTW_PHASE_PROFILE needs the -DRTW_MEASURE build (tools/gpu_phase.sh)");
#endif
  const int r = launch_all(sc, cam, p, workspace, ws_bytes, nullptr, nullptr, nullptr, nullptr, mode);
  if (r != RTW_OK) return r;
  HIP_TRY(hipDeviceSynchronize());
  for (auto& x : st) x = 0;
  const WsLayout L = rtwp::ws_layout(p);
  HIP_TRY(hipMemcpy(st, static_cast<unsigned char*>(workspace) + L.stats_off, sizeof(st), hipMemcpyDeviceToHost));
  if (mode == 1 && dev_knob("RTW_COUNTS_VERBOSE")) {
    fprintf(stderr, "[rtw counts] samples %llu segments %llu skipped %llu cand_wave_iters %llu cand_lanes %llu "
            "disc_ge0_lanes %llu sphere_loop_wave_iters %llu cull_survivor_lanes %llu cull_exact_wave_iters %llu "
            "cluster_wave_tests %llu cluster_wave_skips %llu primary_rounds %llu primary_idle_lanes %llu "
            "mask_popcount_sum %llu\n", st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8],
            st[11], st[12], st[14], st[15], st[16]);
    if (st[13])  // wavefront engine, wf_drain
      fprintf(stderr, "[rtw counts] drain wave iterations %llu, drained segments per wave iteration %.2f of 64\n",
              st[13], (double)st[9] / (double)st[13]);
  }
  if (mode == 2) {
    const char* names[10] = {"refill",  "start_sample", "wide+pretest", "hit+kind",    "tail",
                             "loop_top", "exact_survivors", "coop_ball", "hitrec+scatter", "primary"};
    unsigned long long tot = 0;
    for (int i = 0; i < 10; ++i) tot += st[16 + i];
    for (int i = 0; i < 10; ++i)
      fprintf(stderr, "[rtw phase] %-15s %6.2f%%  (%llu wave-cycles)\n", names[i], tot ? 100.0 * st[16 + i] / tot : 0.0,
              st[16 + i]);
  }
  return RTW_OK;
}

int rtw_render_stats(rtw_scene sc, const rtw_camera* cam, const rtw_params* p, void* workspace, size_t ws_bytes,
                     uint64_t stats_out[RTW_STATS_WORDS]) {
  if (!stats_out) return rtw_fail(RTW_EINVAL, "stats is NULL");
  unsigned long long st[32];
  const int r = stats_pass(sc, cam, p, workspace, ws_bytes, st);
  if (r != RTW_OK) return r;
  for (int i = 0; i < RTW_STATS_WORDS; ++i) stats_out[i] = st[i];
  return RTW_OK;
}

int rtw_render_stats_ex(rtw_scene sc, const rtw_camera* cam, const rtw_params* p, void* workspace, size_t ws_bytes,
                        uint64_t* stats_out, uint32_t n_words) {
  if (!stats_out || n_words > RTW_STATS_WORDS_EX) return rtw_fail(RTW_EINVAL, "stats is NULL or n_words > %d", RTW_STATS_WORDS_EX);
  unsigned long long st[32];
  const int r = stats_pass(sc, cam, p, workspace, ws_bytes, st);
  if (r != RTW_OK) return r;
  for (uint32_t i = 0; i < n_words; ++i) stats_out[i] = st[i];
  return RTW_OK;
}

int rtw_render_counts_ex(rtw_scene sc, const rtw_camera* cam, const rtw_params* p, void* workspace,
                         size_t ws_bytes, uint64_t counts_out[6]) {
  if (!counts_out) return rtw_fail(RTW_EINVAL, "counts is NULL");
  unsigned long long st[32];
  const int r = stats_pass(sc, cam, p, workspace, ws_bytes, st);
  if (r != RTW_OK) return r;
  counts_out[0] = st[0];
  counts_out[1] = st[1];
  // every segment tests every sphere; f32 mode skips one small sphere per segment with a skip set
  counts_out[2] = st[1] * sc->n_static;
  counts_out[3] = st[1] * sc->n_moving;
  if (p->precision == RTW_PRECISION_F32) counts_out[2] -= st[2];
  counts_out[4] = st[9];  // wf_finish (rtw_wavefront.hip shade_step FIN)
  counts_out[5] = st[10];
  return RTW_OK;
}

int rtw_render_counts(rtw_scene sc, const rtw_camera* cam, const rtw_params* p, void* workspace,
                      size_t ws_bytes, uint64_t counts_out[4]) {
  if (!counts_out) return rtw_fail(RTW_EINVAL, "scene/camera/counts is NULL");
  uint64_t c[6];
  const int r = rtw_render_counts_ex(sc, cam, p, workspace, ws_bytes, c);
  if (r == RTW_OK)
    for (int i = 0; i < 4; ++i) counts_out[i] = c[i];
  return r;
}

int rtw_render(const rtw_camera* cam, const rtw_sphere* spheres, uint32_t n, const rtw_material* mats, uint32_t nm,
               const rtw_params* p, uint8_t* rgb_out, float* mean_out) {
  if (!cam || !rgb_out) return rtw_fail(RTW_EINVAL, "camera/rgb_out is NULL");
  const int v = rtw_validate_params(p);
  if (v != RTW_OK) return v;
  RtwOneShot o;
  int st = o.enter(p);
  if (st != RTW_OK) return st;
  rtw_scene sc = nullptr;
  st = rtw_scene_create(spheres, n, mats, nm, &sc);
  if (st == RTW_OK) st = o.alloc("rtw_render", rtwp::ws_layout(p).total, p, mean_out != nullptr);
  hipStream_t s = nullptr;
  if (st == RTW_OK && hipStreamCreate(&s) != hipSuccess) st = rtw_fail(RTW_EHIP, "hipStreamCreate failed");
  if (st == RTW_OK) st = launch_all(sc, cam, p, o.ws, o.ws_bytes, o.d_rgb, o.d_mean, s, nullptr, 0);
  if (st == RTW_OK && hipStreamSynchronize(s) != hipSuccess) st = rtw_fail(RTW_EHIP, "render failed on the device");
  if (st == RTW_OK) st = o.copy_back(rgb_out, mean_out);
  if (s) (void)hipStreamDestroy(s);
  rtw_scene_destroy(sc);
  return st;
}

}  // extern "C"

// ---- shared with the other files of the C ABI (rtw_capi_shared.hpp) ----
const char* rtw_dev_knob(const char* name) { return dev_knob(name); }
int rtw_device_cus(int dev) { return device_cus(dev); }
int rtw_wf_blocks_per_cu(int dev, int prec, int kernel, size_t lds) {
  std::lock_guard<std::mutex> lk(g_dev_mu);
  auto& e = g_dev[dev].bpc[{prec, -kernel}];
  if (e.second == 0 || e.first != lds) e = {lds, rtwk::wf_blocks_per_cu(prec, kernel, lds)};
  return e.second;
}

int rtw_launch_begin(const WsLayout& L, void* ws, size_t ws_bytes, int owner_device, const char* mismatch_fmt,
                     rtw_accum acc, rtw_timer timer, hipStream_t stream, int* dev, RtwPassMap* map, bool* launch) {
  *launch = true;
  if (!ws || ws_bytes < L.total) return rtw_fail(RTW_EINVAL, "workspace %zu bytes < required %zu", ws_bytes, L.total);
  if ((reinterpret_cast<uintptr_t>(ws) & 255) != 0) return rtw_fail(RTW_EINVAL, "workspace not 256-B aligned");
  HIP_TRY(hipGetDevice(dev));
  if (*dev != owner_device) return rtw_fail(RTW_EINVAL, mismatch_fmt, owner_device, *dev);
  if (acc) {
    const int st = rtw_accum_pass_map(acc, map);
    if (st != RTW_OK) return st;
    if (map->list && map->tiles == 0) {  // nothing launched: the timer holds no interval (not the previous pass's)
      if (timer) timer->recorded = false;
      *launch = false;
      return RTW_OK;
    }
  }
  HIP_TRY(hipMemsetAsync(static_cast<unsigned char*>(ws) + L.counter_off, 0, L.counter_bytes, stream));
  return RTW_OK;
}

int RtwOneShot::enter(const rtw_params* p) {
  int ndev = 0, cur = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return rtw_fail(RTW_ENODEV, "no HIP device visible");
  HIP_TRY(hipGetDevice(&cur));
  const int dev = p->device < 0 ? cur : p->device;
  if (dev >= ndev) return rtw_fail(RTW_EINVAL, "device %d >= device count %d", dev, ndev);
  HIP_TRY(hipSetDevice(dev));
  prev = cur;
  return RTW_OK;
}
int RtwOneShot::alloc(const char* who, size_t workspace_bytes, const rtw_params* p, bool mean) {
  ws_bytes = workspace_bytes;
  pix = (size_t)p->row_count * p->width * 3;
  if (hipMalloc(&ws, ws_bytes) != hipSuccess || hipMalloc(&d_rgb, pix) != hipSuccess ||
      (mean && hipMalloc(&d_mean, pix * sizeof(float)) != hipSuccess))
    return rtw_fail(RTW_ENOMEM, "%s: device allocation failed", who);
  return RTW_OK;
}
int RtwOneShot::copy_back(uint8_t* rgb_out, float* mean_out) const {
  if (hipMemcpy(rgb_out, d_rgb, pix, hipMemcpyDeviceToHost) != hipSuccess)
    return rtw_fail(RTW_EHIP, "copy of rgb_out failed");
  if (mean_out && hipMemcpy(mean_out, d_mean, pix * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
    return rtw_fail(RTW_EHIP, "copy of mean_out failed");
  return RTW_OK;
}
RtwOneShot::~RtwOneShot() {
  if (ws) (void)hipFree(ws);
  if (d_rgb) (void)hipFree(d_rgb);
  if (d_mean) (void)hipFree(d_mean);
  if (prev >= 0) (void)hipSetDevice(prev);
}

void rtw_fill_trace_args(rtwk::TraceArgs<double>& a, const rtw_camera* cam, const rtw_params* p, unsigned char* ws,
                         uint64_t seed_adv) {
  fill_args(a, rtwk::SceneView<double>{}, cam, p, ws, rtwp::ws_layout(p), seed_adv);
  a.unit_order = unit_order(kWorldUnitOrder);  // the world kernel's default (fill_args)
}
int rtw_launch_finalize(const rtw_params* p, unsigned char* ws, uint8_t* d_rgb, float* d_mean, hipStream_t s) {
  const WsLayout L = rtwp::ws_layout(p);
  rtwk::FinalizeArgs f;
  f.partial = reinterpret_cast<const double*>(ws + L.partial_off);
  f.rgb = d_rgb;
  f.mean = d_mean;
  f.npix = p->row_count * p->width;
  f.n_chunks = rtwp::n_chunks(p);
  f.scale = 1.0 / (double)p->spp;
  const hipError_t e = rtwk::launch_finalize(f, s);
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "finalize kernel launch: %s", hipGetErrorString(e));
  return RTW_OK;
}
int rtw_timer_mark(rtw_timer t, hipStream_t s, bool start) {
  if (hipEventRecord(start ? t->start : t->stop, s) != hipSuccess) return rtw_fail(RTW_EHIP, "timer event record failed");
  if (!start) t->recorded = true;
  return RTW_OK;
}
