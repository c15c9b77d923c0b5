// rtw_capi.hip — the C ABI (include/rtw_hip.h): validation, scene upload,
// workspace sizing, kernel launches.  Replaces the render loop of
// src/main.zig:378-402.  No exception and no C++ type crosses the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
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
#include "rtw_internal.hpp"
#include "rtw_math.hpp"
#include "rtw_scene_pack.hpp"

namespace {

thread_local std::string g_err;

int fail(int status, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return status;
}
#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) return fail(RTW_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

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

struct DevInfo {
  int cus = 0;
  std::map<std::pair<int, int>, std::pair<size_t, int>> bpc;  // (precision, var) -> (lds, blocks per CU)
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
int blocks_per_cu(int dev, int prec, size_t lds, int var) {
  std::lock_guard<std::mutex> lk(g_dev_mu);
  auto& d = g_dev[dev];
  auto& e = d.bpc[{prec, var}];
  if (e.second == 0 || e.first != lds) e = {lds, rtwk::trace_blocks_per_cu(prec, lds, var)};
  return e.second;
}
// Wavefront bounce kernels: resident workgroups per CU (cached per device).
int wf_bpc(int dev, int prec, int kernel, size_t lds) {
  std::lock_guard<std::mutex> lk(g_dev_mu);
  auto& e = g_dev[dev].bpc[{prec, -kernel}];
  if (e.second == 0 || e.first != lds) e = {lds, rtwk::wf_blocks_per_cu(prec, kernel, lds)};
  return e.second;
}
// Kernel tuning variant (rtw_trace.hip VAR bits): the product library holds
// one per precision (rtw_internal.hpp kDefaultVarF64 / kDefaultVarF32).
// RTW_VARIANT selects another one of a -DRTW_MEASURE build (tools/); a value
// that was not compiled in is refused by launch_all.
int kernel_variant(uint32_t precision) {
  const char* v = dev_knob("RTW_VARIANT");
  if (v && *v) return atoi(v);
  return precision == RTW_PRECISION_F32 ? rtwk::kDefaultVarF32 : rtwk::kDefaultVarF64;
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
  if (!out) return fail(RTW_EINVAL, "rtw_scene_create: out is NULL");
  *out = nullptr;
  rtwp::ScenePack k;
  std::string msg;
  const int st = rtwp::pack_scene(spheres, n, mats, nm, k, msg);
  if (st != RTW_OK) return fail(st, "%s", msg.c_str());
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  const size_t total = k.blob.size();
  void* d = nullptr;
  if (hipMalloc(&d, total) != hipSuccess) return fail(RTW_ENOMEM, "rtw_scene_create: hipMalloc(%zu)", total);
  if (hipMemcpy(d, k.blob.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return fail(RTW_EHIP, "rtw_scene_create: hipMemcpy failed");
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

namespace {

uint32_t eff_chunk(const rtw_params* p) {
  const uint32_t c = p->chunk ? p->chunk : RTW_DEFAULT_CHUNK;
  return std::min(c, p->spp);
}
uint32_t n_chunks(const rtw_params* p) {
  const uint32_t c = eff_chunk(p);
  return (p->spp + c - 1) / c;
}

int validate(const rtw_params* p) {
  if (!p) return fail(RTW_EINVAL, "params is NULL");
  if (p->width < 2 || p->height < 2)
    return fail(RTW_EINVAL, "image %ux%u: width and height must be >= 2 (main.zig:390-391 divide by W-1, H-1)",
                p->width, p->height);
  if (p->spp == 0) return fail(RTW_EINVAL, "spp must be >= 1");
  if ((uint64_t)p->width * p->height > (1ull << 24))
    return fail(RTW_UNSUPPORTED, "image of %llu pixels exceeds 2^24 (per-sample RNG key layout)",
                (unsigned long long)p->width * p->height);
  if (p->spp > (1u << 24)) return fail(RTW_UNSUPPORTED, "spp %u exceeds 2^24", p->spp);
  if (p->row_stride == 0 || p->row_count == 0) return fail(RTW_EINVAL, "row_stride and row_count must be >= 1");
  if ((uint64_t)p->row_begin + (uint64_t)(p->row_count - 1) * p->row_stride >= p->height)
    return fail(RTW_EINVAL, "rows %u + k*%u (k < %u) exceed height %u", p->row_begin, p->row_stride,
                p->row_count, p->height);
  if (p->precision > RTW_PRECISION_F32) return fail(RTW_EINVAL, "precision %u", p->precision);
  if (p->engine > RTW_ENGINE_WAVEFRONT) return fail(RTW_EINVAL, "engine %u", p->engine);
  if (p->wf_sets > RTW_MAX_WF_SETS) return fail(RTW_EINVAL, "wf_sets %u outside [0, %u]", p->wf_sets, RTW_MAX_WF_SETS);
  if (p->wf_drain > RTW_WF_DRAIN_NONE) return fail(RTW_EINVAL, "wf_drain %u", p->wf_drain);
  if (p->wf_form > RTW_WF_SPLIT) return fail(RTW_EINVAL, "wf_form %u", p->wf_form);
  if (p->world_waves > 4 || p->world_waves == 2)  // (compiled budgets: 1 = unconstrained, 3, 4)
    return fail(RTW_EINVAL, "world_waves %u is not 0, 1, 3 or 4", p->world_waves);
  if (p->world_features > RTW_WORLD_FEATURES_ALL) return fail(RTW_EINVAL, "world_features %u", p->world_features);
  if (p->world_traversal > RTW_WORLD_TRAVERSAL_LANE) return fail(RTW_EINVAL, "world_traversal %u", p->world_traversal);
  if (p->wf_bounces > 16) return fail(RTW_EINVAL, "wf_bounces %u outside [0, 16]", p->wf_bounces);
  if (p->wf_passes > 64) return fail(RTW_EINVAL, "wf_passes %u outside [0, 64]", p->wf_passes);
  if (p->engine == RTW_ENGINE_WAVEFRONT && (p->wf_paths > (1u << 28) || (p->wf_paths && p->wf_paths < 64)))
    return fail(RTW_EINVAL, "wf_paths %u outside [64, 2^28]", p->wf_paths);
  if (p->engine == RTW_ENGINE_WAVEFRONT && p->max_depth > 0xFFFFu)
    return fail(RTW_UNSUPPORTED, "wavefront engine: max_depth %u > 65535", p->max_depth);
  const uint64_t tiles = (uint64_t)((p->width + rtwk::kTileW - 1) / rtwk::kTileW) *
                         ((p->row_count + rtwk::kTileH - 1) / rtwk::kTileH);
  const uint64_t units = tiles * 64ull * n_chunks(p);
  if (units > 0x7FFFFFFFull)  // headroom: waves overshoot the queue by < 2^31 units
    return fail(RTW_UNSUPPORTED, "%llu work units exceed the 32-bit queue; raise params.chunk",
                (unsigned long long)units);
  return RTW_OK;
}

// Wavefront queue sets (params.wf_sets, default kWfSets): the in-flight paths
// are split over independent sets (queues, home slots, segment counts,
// reservoirs, drain ring), each driven on its own HIP stream, so one set's
// launch ramps, tails and drain overlap the other sets' bounce launches.  All
// sets take units from the one device queue: a unit belongs to one slot of
// one set, its chunk sum keeps its sample order, the image keeps its bits.
constexpr uint32_t kWfMaxSets = RTW_MAX_WF_SETS;
constexpr uint32_t kWfSets = RTW_DEFAULT_WF_SETS;
uint32_t wf_sets(const rtw_params* p) { return p->wf_sets ? p->wf_sets : kWfSets; }  // (validated: 1-4)
// The in-register drain (params.wf_drain): wf_drain (RTW_WF_DRAIN_SAMPLES,
// samples dealt to the wave's free lanes, default), wf_finish
// (RTW_WF_DRAIN_SLOTS: a lane runs its own slot's samples) or none.  Only
// wf_drain uses the drain ring, so only it reserves one.
bool wf_per_sample_drain(const rtw_params* p) { return p->wf_drain == RTW_WF_DRAIN_SAMPLES; }
// Segments of one queue set: its share of wf_paths rounded up to whole
// segments (one per wave).
uint32_t wf_segs(const rtw_params* p) {
  const uint32_t n = p->wf_paths ? p->wf_paths : RTW_DEFAULT_WF_PATHS;
  const uint32_t per_set = (n + wf_sets(p) - 1) / wf_sets(p);
  return std::max(1u, (per_set + rtwk::kSegCap - 1) / rtwk::kSegCap);
}

// Workspace: partial chunk sums | counters (unit queue head, one live-path
// poll word per queue set) | stats | wavefront region (engine 1 only,
// rtw_internal.hpp WfArgs): per queue set two path queues, the hit arrays,
// the home slots, per-segment counts (x2), unit reservoirs and (wf_drain
// only) the drain ring.
struct WsLayout {
  size_t partial_off, partial_bytes, counter_off, live_off, stats_off;
  size_t wf_off, wf_set_bytes, total;
};
size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
// Byte size of one SoA path queue of n entries (10 R arrays, rs, slot, dsk, + the fused engine's hit root, winner).
// (10 R fields, the RNG state, slot, depth|skip, the fused engine's hit winner; round 6 dropped the
// hit root: a queued hit path carries its hit point in o)
size_t wf_queue_bytes(size_t n, size_t r) { return 10 * al256(n * r) + al256(n * 8) + 3 * al256(n * 4); }
WsLayout ws_layout(const rtw_params* p) {
  WsLayout w;
  w.partial_off = 0;
  w.partial_bytes = (size_t)n_chunks(p) * p->row_count * p->width * 3 * sizeof(double);
  w.counter_off = al256(w.partial_bytes);
  w.live_off = w.counter_off + 64;  // kWfMaxSets words; + 128: wf_step's live_acc pairs (kWfMaxSets x 2 words)
  w.stats_off = w.counter_off + 256;
  w.total = w.stats_off + 256;  // stats: 32 x u64
  w.wf_off = w.total;
  w.wf_set_bytes = 0;
  if (p->engine == RTW_ENGINE_WAVEFRONT) {
    const size_t segs = wf_segs(p), n = segs * rtwk::kSegCap;
    const size_t r = p->precision == RTW_PRECISION_F32 ? 4 : 8;
    w.wf_set_bytes = 2 * wf_queue_bytes(n, r) + al256(n * r) + al256(n * 4) + al256(n * sizeof(rtwk::HomeRec)) +
                     2 * al256(segs * 4) + al256(segs * 8) +
                     (wf_per_sample_drain(p) ? al256(n * rtwk::kDrainWin * 3 * r) : 0);
    w.total += wf_sets(p) * w.wf_set_bytes;
  }
  return w;
}

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
  a.chunk = eff_chunk(p);
  a.n_chunks = n_chunks(p);
  a.row_begin = p->row_begin;
  a.row_stride = p->row_stride;
  a.row_count = p->row_count;
  a.tiles_x = (p->width + rtwk::kTileW - 1) / rtwk::kTileW;
  const uint32_t tiles_y = (p->row_count + rtwk::kTileH - 1) / rtwk::kTileH;
  a.total_units = a.tiles_x * tiles_y * 64u * a.n_chunks;
  const rtwm::UDivMagic mu = rtwm::udiv_magic(rtwk::kTileW * rtwk::kTileH * a.n_chunks), mt = rtwm::udiv_magic(a.tiles_x);
  a.upt_m = mu.m, a.upt_sh = mu.sh, a.tx_m = mt.m, a.tx_sh = mt.sh;
  // seed_adv: 0 for a frame; an accumulator pass starts at sample s0 of its
  // pixels' streams, s0 * (gamma << 16) further on (accum_pass_begin).
  a.seed_base = splitmix_first(p->seed) + seed_adv;
  // Unit dealing order (rtw_device.hpp dealt_unit): image order, top rows
  // first, for the cover-scene engines, last-first for the world kernel
  // (rtw_fill_trace_args), each the faster in the in-process A/Bs
  // (profiles/r03/unit_order_ab.txt); RTW_UNIT_ORDER=fwd|rev overrides.
  a.unit_order = unit_order(0u);
  a.partial = reinterpret_cast<double*>(ws + L.partial_off);
  a.counter = reinterpret_cast<uint32_t*>(ws + L.counter_off);
  a.stats = reinterpret_cast<unsigned long long*>(ws + L.stats_off);
}

// n_clusters: clusters whose slot -> position table (cpos) is staged, 0 unless
// the launched kernel runs the clustered pretest (f64 megakernel with
// kVarCluster and clusters_usable): other paths neither read nor stage it.
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

// ---------------------------------------------------------- wavefront ----
template <typename R>
rtwk::PathBuf<R> carve_queue(unsigned char*& b, size_t n) {
  rtwk::PathBuf<R> q;
  R** arr[10] = {&q.ox, &q.oy, &q.oz, &q.dx, &q.dy, &q.dz, &q.tx, &q.ty, &q.tz, &q.tm};
  for (R** a : arr) {
    *a = reinterpret_cast<R*>(b);
    b += al256(n * sizeof(R));
  }
  q.rs = reinterpret_cast<uint64_t*>(b);
  b += al256(n * 8);
  q.slot = reinterpret_cast<uint32_t*>(b);
  b += al256(n * 4);
  q.dsk = reinterpret_cast<uint32_t*>(b);
  b += al256(n * 4);
  q.hk = reinterpret_cast<int32_t*>(b);
  b += al256(n * 4);
  return q;
}

// Thread-local pinned words the host polls for the queue lengths (two per
// queue set: batches are checked one behind).
// Mapped: the fused engine's wf_step writes its batch's word from the device
// (poll_words_dev: the device address of the same words).
uint32_t* poll_words() {
  thread_local uint32_t* w = nullptr;
  if (!w && hipHostMalloc(reinterpret_cast<void**>(&w), 4 * kWfMaxSets * sizeof(uint32_t),
                          hipHostMallocPortable | hipHostMallocMapped) != hipSuccess)
    w = nullptr;
  return w;
}
uint32_t* poll_words_dev(uint32_t* host) {
  void* d = nullptr;
  return host && hipHostGetDevicePointer(&d, host, 0) == hipSuccess ? static_cast<uint32_t*>(d) : nullptr;
}

// Side streams of the wavefront queue sets 1.. (set 0 runs on the caller's
// stream): created once per device for the whole process (not per host
// thread, so a process does not accumulate streams beyond the hardware
// queues, where HIP would map them round-robin onto shared queues and a set
// could land on its caller's queue — correct, but serial); non-blocking,
// joined to the caller's stream by events on every render; kept for the
// life of the process.  Concurrent wavefront renders on one device from several
// threads share them (stream-ordered: still correct).
// The streams live for the process and are never destroyed: a
// static destructor would run during exit, possibly after the HIP runtime's
// own teardown (registered at the first HIP call, after this object was
// constructed), where hipStreamDestroy may crash or hang.  The runtime
// releases them with the process.
struct SideStreams {
  std::mutex mu;
  std::map<std::pair<int, uint32_t>, hipStream_t> s;
};
SideStreams& g_side = *new SideStreams;  // (leaked on purpose: no exit-time destructor)
hipStream_t wf_side_stream(int dev, uint32_t k) {
  std::lock_guard<std::mutex> lk(g_side.mu);
  hipStream_t& s = g_side.s[{dev, k}];
  if (!s) {
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess || cur != dev ||
        hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess)
      s = nullptr;
  }
  return s;
}

// One queue set of the wavefront engine: its region of the workspace, its
// stream and its host-side progress.
template <typename R>
struct WfSet {
  rtwk::WfArgs<R> a;
  rtwk::PathBuf<R> qa, qb;
  uint32_t *seg_a = nullptr, *seg_b = nullptr;
  hipStream_t s = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  uint64_t batch = 0;
  bool done = false;
  bool started = false;  // its generate kernel was enqueued
};

// Wavefront render: per queue set, generate, then batches of kWfIters bounce
// launches; after each batch wf_count sums the segment counts of the set's
// queue A and the total is copied to pinned memory.  The host stops a set
// once a batch (checked one batch behind, so the GPU never idles on the poll)
// left its queue empty, or hands the set's drain to wf_drain / wf_finish once
// its live count shows retiring slots.  Empty batches cost only the
// launches: every wave reads its count first.  Sets run on their own streams,
// forked from and joined back to the caller's stream.
constexpr uint32_t kWfBatch = 64;
constexpr int kWfIters = 8;  // even: each batch ends with the live paths in queue A
template <typename R>
int run_wavefront(const rtwk::TraceArgs<R>& ta, const rtw_params* p, unsigned char* ws, const WsLayout& L, int dev,
                  size_t lds, hipStream_t stream, bool stats) {
  if (ta.max_depth == 0) {  // rayColor(depth 0) is black (main.zig:105-108): no segment to trace
    HIP_TRY(hipMemsetAsync(ws + L.partial_off, 0, L.partial_bytes, stream));
    return RTW_OK;
  }
  const uint32_t segs = wf_segs(p), nsets = wf_sets(p);
  const size_t n = (size_t)segs * rtwk::kSegCap;
  const bool per_sample = wf_per_sample_drain(p);
  // Units per reservoir refill (kWfBatch; development knob RTW_WF_BATCH): the
  // refills' atomics against the work a reservoir still holds when the queue
  // runs dry.
  const char* be = dev_knob("RTW_WF_BATCH");
  const uint32_t refill = (be && *be) ? (uint32_t)std::max(1, atoi(be)) : kWfBatch;
  // Bounce segments per path per wf_step launch (params.wf_bounces, 0 = 1):
  // the path stays in registers between them.
  const uint32_t bounces = p->wf_bounces ? p->wf_bounces : 1u;
  // Persistent grids: every resident wave slot of each bounce kernel (at most
  // one wave per segment); the same grids for every launch of the frame.
  // The drains always run max_grid = ceil(segs / waves per block) blocks: one
  // wave per segment (wf_drain has no segment loop; grid_of never sizes them).
  const uint32_t max_grid = (segs + rtwk::kTraceBlock / 64 - 1) / (rtwk::kTraceBlock / 64);
  // RTW_WF_GRID (development knob): N > 0 = N x the resident grid, capped at one wave per segment.
  const char* gk = dev_knob("RTW_WF_GRID");
  const uint32_t gmul = (gk && *gk) ? (uint32_t)std::max(1, atoi(gk)) : 1u;
  // RTW_WF_SET_GRID (development knob): each set's bounce grid = the resident grid / N.
  const char* sg = dev_knob("RTW_WF_SET_GRID");
  const uint32_t gdiv = (sg && *sg) ? (uint32_t)std::max(1, atoi(sg)) : 1u;
  auto grid_of = [&](int kernel) {
    const uint32_t per_cu = (uint32_t)wf_bpc(dev, (int)(sizeof(R) == 4), kernel, lds);
    return std::max(1u, std::min((uint32_t)device_cus(dev) * per_cu * gmul / gdiv, max_grid));
  };
  const uint32_t grid = grid_of(2), grid_ext = grid_of(1), grid_step = grid_of(3);
  // Fused engine (default; params.wf_form RTW_WF_SPLIT: separate extend and
  // shade kernels): one kernel per bounce, the closest hit computed where the
  // ray is made.
  const bool fused = p->wf_form == RTW_WF_FUSED;
  // Queue passes per wf_step launch (params.wf_passes, fused form): each pass
  // moves every path through the queues; a batch holds >= kWfIters passes.
  const uint32_t passes = !fused ? 1u : p->wf_passes ? p->wf_passes : RTW_DEFAULT_WF_PASSES;
  const int iters = std::max(2, (kWfIters / (int)passes) & ~1);  // even: the batch ends with the paths in queue A
  uint32_t* poll = poll_words();
  if (!poll) return fail(RTW_EHIP, "hipHostMalloc of the poll words failed");
  uint32_t* poll_dev = poll_words_dev(poll);
  if (!poll_dev) return fail(RTW_EHIP, "hipHostGetDevicePointer of the poll words failed");
  // development knobs: RTW_WF_POLL_KERNEL=1 polls the fused engine through
  // wf_count + copy as the split form does; RTW_WF_POLL_CHECK=1 runs both and
  // reports on stderr a batch whose published count differs from wf_count's
  const char* pk = dev_knob("RTW_WF_POLL_KERNEL");
  const char* pc = dev_knob("RTW_WF_POLL_CHECK");
  const bool poll_check = fused && pc && *pc == '1';
  const bool publish = fused && !(pk && *pk == '1');
  if (publish && grid_step >= (1u << 20)) return fail(RTW_EINVAL, "wf_step grid %u exceeds the poll ticket's 20 bits", grid_step);
  WfSet<R> set[kWfMaxSets];
  int st = RTW_OK;
  hipEvent_t fork = nullptr;
  if (hipEventCreateWithFlags(&fork, hipEventDisableTiming) != hipSuccess || hipEventRecord(fork, stream) != hipSuccess)
    st = fail(RTW_EHIP, "wavefront fork event failed");
  for (uint32_t k = 0; k < nsets && st == RTW_OK; ++k) {
    WfSet<R>& S = set[k];
    rtwk::WfArgs<R>& a = S.a;
    std::memset(&a, 0, sizeof(a));
    a.t = ta;
    unsigned char* b = ws + L.wf_off + k * L.wf_set_bytes;
    S.qa = carve_queue<R>(b, n);
    S.qb = carve_queue<R>(b, n);
    auto take = [&](size_t bytes) {
      unsigned char* q = b;
      b += al256(bytes);
      return q;
    };
    a.hit_t = reinterpret_cast<R*>(take(n * sizeof(R)));
    a.hit_k = reinterpret_cast<int32_t*>(take(n * 4));
    a.home = reinterpret_cast<rtwk::HomeRec*>(take(n * sizeof(rtwk::HomeRec)));
    S.seg_a = reinterpret_cast<uint32_t*>(take(segs * 4));
    S.seg_b = reinterpret_cast<uint32_t*>(take(segs * 4));
    a.seg_resv = reinterpret_cast<uint32_t*>(take(segs * 8));
    a.drain_buf = per_sample ? reinterpret_cast<R*>(take(n * rtwk::kDrainWin * 3 * sizeof(R))) : nullptr;
    a.live = reinterpret_cast<uint32_t*>(ws + L.live_off) + k;
    a.n_slots = (uint32_t)n;
    a.n_segs = segs;
    a.batch = refill;
    a.bounces = bounces;
    a.passes = passes;
    a.hit_form = fused ? 1u : 0u;  // fused: queued paths carry their hit (hk, o = the hit point)
    a.live_acc = reinterpret_cast<uint32_t*>(ws + L.counter_off + 128) + 2 * k;  // (zeroed with the queue head)
    a.poll_out = nullptr;  // (set per batch)
    S.s = k == 0 ? stream : wf_side_stream(dev, k);  // (set 0: the caller's stream, NULL = the default stream)
    if (k > 0 && !S.s) {
      st = fail(RTW_EHIP, "wavefront side stream creation failed");
      break;
    }
    for (auto& x : S.ev)
      if (hipEventCreateWithFlags(&x, hipEventDisableTiming) != hipSuccess) st = fail(RTW_EHIP, "hipEventCreate failed");
    if (st != RTW_OK) break;
    if (k > 0 && hipStreamWaitEvent(S.s, fork, 0) != hipSuccess) {
      st = fail(RTW_EHIP, "wavefront fork wait failed");
      break;
    }
    // generate -> queue A
    a.out = S.qa;
    a.seg_out = S.seg_a;
    const hipError_t e =
        fused ? rtwk::launch_wf_generate_hit(a, grid_step, lds, S.s) : rtwk::launch_wf_generate(a, grid, 0, S.s);
    if (e != hipSuccess) st = fail(RTW_EHIP, "wavefront generate launch: %s", hipGetErrorString(e));
    S.started = true;
  }
  // Termination bound (never reached by a correct kernel): every iteration
  // advances every live path by one segment.
  const uint64_t max_batches = (uint64_t)ta.total_units * ta.chunk * (ta.max_depth + 1ull) / (uint64_t)(iters * passes) + 4;
  // Wall-clock guard as well (300 s; development knob RTW_WF_TIMEOUT_S): a
  // queue that never drains is reported instead of hanging the caller.
  const char* tos = dev_knob("RTW_WF_TIMEOUT_S");
  const double timeout_s = (tos && *tos) ? atof(tos) : 300.0;
  const auto t_start = std::chrono::steady_clock::now();
  // Drain in registers once a set's polled live count falls below fin_frac x
  // its slots: 1 as soon as slots start to retire, i.e. the unit queue ran
  // dry; 0 with RTW_WF_DRAIN_NONE (through the queues to the end); the
  // development knob RTW_WF_FINISH sets another fraction.
  const char* fe = dev_knob("RTW_WF_FINISH");
  const double fin_frac = p->wf_drain == RTW_WF_DRAIN_NONE ? 0.0 : (fe && *fe) ? atof(fe) : 1.0;
  uint32_t left = st == RTW_OK ? nsets : 0u;
  while (left > 0 && st == RTW_OK) {
    // Enqueue one batch on every running set, then look at each set's
    // previous batch (so every stream holds a batch while the host waits).
    for (uint32_t k = 0; k < nsets && st == RTW_OK; ++k) {
      WfSet<R>& S = set[k];
      if (S.done) continue;
      rtwk::WfArgs<R>& a = S.a;
      hipError_t e = hipSuccess;
      // fused: the batch's wf_step launches publish the live count into this
      // batch's pinned word themselves (wf_step publish_live); split: wf_count + copy
      a.poll_out = publish ? poll_dev + 2 * k + (S.batch & 1) : nullptr;
      for (int i = 0; i < iters && e == hipSuccess; ++i) {
        const bool even = (i & 1) == 0 || (passes & 1u) == 0u;  // (an even pass count returns to its input queue)
        a.in = even ? S.qa : S.qb;
        a.out = even ? S.qb : S.qa;
        a.seg_in = even ? S.seg_a : S.seg_b;
        a.seg_out = even ? S.seg_b : S.seg_a;
        if (fused)
          e = rtwk::launch_wf_step(a, grid_step, lds, S.s, stats);
        else if ((e = rtwk::launch_wf_extend(a, grid_ext, lds, S.s)) == hipSuccess)
          e = rtwk::launch_wf_shade(a, grid, lds, S.s, stats);
      }
      if (e != hipSuccess) {
        st = fail(RTW_EHIP, "wavefront bounce launch: %s", hipGetErrorString(e));
        break;
      }
      uint32_t* pw = poll + (publish ? 2 * kWfMaxSets : 0u) + 2 * k + (S.batch & 1);
      if (((!publish || poll_check) && (rtwk::launch_wf_count(S.seg_a, segs, a.live, S.s) != hipSuccess ||
                      hipMemcpyAsync(pw, a.live, 4, hipMemcpyDeviceToHost, S.s) != hipSuccess)) ||
          hipEventRecord(S.ev[S.batch & 1], S.s) != hipSuccess)
        st = fail(RTW_EHIP, "wavefront poll enqueue failed");
      a.poll_out = nullptr;  // (the drains and checks below do not publish)
    }
    for (uint32_t k = 0; k < nsets && st == RTW_OK; ++k) {
      WfSet<R>& S = set[k];
      if (S.done) continue;
      const uint64_t b = S.batch++;
      if (b == 0) continue;
      if (hipEventSynchronize(S.ev[(b - 1) & 1]) != hipSuccess) {
        st = fail(RTW_EHIP, "wavefront batch failed on the device");
        break;
      }
      const uint32_t live = poll[2 * k + ((b - 1) & 1)];
      if (poll_check && publish && live != poll[2 * kWfMaxSets + 2 * k + ((b - 1) & 1)])
        std::fprintf(stderr, "[rtw wf poll] set %u batch %llu: published %u, wf_count %u\n", k,
                     (unsigned long long)(b - 1), live, poll[2 * kWfMaxSets + 2 * k + ((b - 1) & 1)]);
      if (live != 0u && (double)live < fin_frac * (double)n) {  // queue A holds the paths after this batch
        rtwk::WfArgs<R>& a = S.a;
        a.in = S.qa;
        a.seg_in = S.seg_a;
        const hipError_t e = per_sample ? rtwk::launch_wf_drain(a, max_grid, lds, S.s, stats)
                                        : rtwk::launch_wf_finish(a, max_grid, lds, S.s, stats);
        if (e != hipSuccess) st = fail(RTW_EHIP, "wavefront finish launch: %s", hipGetErrorString(e));
      }
      if (live == 0u || (double)live < fin_frac * (double)n) {
        S.done = true;
        --left;
      } else if (b > max_batches ||
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() > timeout_s) {
        st = fail(RTW_EHIP, "wavefront queue did not drain after %llu batches", (unsigned long long)b);
      }
    }
  }
  // Every unit must have run: the drains ran outside the batch guard above,
  // so check each set's end state on the device, then join its stream.
  for (uint32_t k = 0; k < nsets; ++k) {
    WfSet<R>& S = set[k];
    if (!S.started) continue;
    if (st == RTW_OK) {
      if (rtwk::launch_wf_check_drained(S.seg_a, S.a.seg_resv, segs, ta.counter, ta.total_units, S.a.live, S.s) !=
              hipSuccess ||
          hipMemcpyAsync(&poll[2 * k], S.a.live, 4, hipMemcpyDeviceToHost, S.s) != hipSuccess ||
          !S.ev[0] || hipEventRecord(S.ev[0], S.s) != hipSuccess)
        st = fail(RTW_EHIP, "wavefront drain check failed to run");
    }
    if (k > 0 && S.ev[1]) {  // join: the caller's stream waits for this set
      if (hipEventRecord(S.ev[1], S.s) != hipSuccess || hipStreamWaitEvent(stream, S.ev[1], 0) != hipSuccess) {
        (void)hipStreamSynchronize(S.s);
        if (st == RTW_OK) st = fail(RTW_EHIP, "wavefront join failed");
      }
    }
  }
  for (uint32_t k = 0; k < nsets && st == RTW_OK; ++k) {
    if (hipEventSynchronize(set[k].ev[0]) != hipSuccess)
      st = fail(RTW_EHIP, "wavefront drain check failed to run");
    else if (poll[2 * k] != 0u)
      st = fail(RTW_EHIP, "wavefront drain of set %u left %u segments/reservoirs with work undone", k, poll[2 * k]);
  }
  for (uint32_t k = 0; k < nsets; ++k)
    for (auto& x : set[k].ev)
      if (x) (void)hipEventDestroy(x);
  if (fork) (void)hipEventDestroy(fork);
  return st;
}

// acc: the render is a pass of this accumulator (p->spp = the pass's samples,
// seed_adv = its offset into the pixels' sample streams): the fold takes the
// place of the finalize launch, ordered as that launch is — on `stream`,
// which the wavefront engine's queue sets have joined by then.
int launch_all(rtw_scene sc, const rtw_camera* cam, const rtw_params* p, void* workspace, size_t ws_bytes,
               uint8_t* d_rgb, float* d_mean, hipStream_t stream, rtw_timer timer, int mode,
               uint64_t seed_adv = 0, rtw_accum acc = nullptr) {
  const WsLayout L = ws_layout(p);
  if (!workspace || ws_bytes < L.total)
    return fail(RTW_EINVAL, "workspace %zu bytes < required %zu", ws_bytes, L.total);
  if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0) return fail(RTW_EINVAL, "workspace not 256-B aligned");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != sc->device)
    return fail(RTW_EINVAL, "scene lives on device %d but the current device is %d", sc->device, dev);
  auto* ws = static_cast<unsigned char*>(workspace);
  // A pass of a masked accumulator deals its active tiles only (TraceArgs::tile_list); with none it
  // launches nothing and changes nothing.
  const uint32_t* m_list = nullptr;
  const uint64_t* m_mask = nullptr;
  uint32_t m_tiles = 0;
  if (acc) {
    const int st = rtw_accum_pass_map(acc, &m_list, &m_mask, &m_tiles);
    if (st != RTW_OK) return st;
    if (m_list && m_tiles == 0) {  // nothing launched: the timer holds no interval (not the previous pass's)
      if (timer) timer->recorded = false;
      return RTW_OK;
    }
  }
  auto mask_args = [&](auto& a) {
    if (!m_list) return;
    a.tile_list = m_list;
    a.tile_mask = m_mask;
    a.total_units = m_tiles * 64u * a.n_chunks;
  };
  HIP_TRY(hipMemsetAsync(ws + L.counter_off, 0, 512, stream));  // queue head + stats
  const int var = (m_list && p->engine == RTW_ENGINE_MEGAKERNEL)
                      ? (p->precision == RTW_PRECISION_F32 ? rtwk::kMaskedVarF32 : rtwk::kMaskedVarF64)
                      : kernel_variant(p->precision);
  if (p->engine != RTW_ENGINE_WAVEFRONT && !rtwk::trace_variant_built((int)p->precision, var))
    return fail(RTW_EINVAL, "RTW_VARIANT=%d: trace kernel variant not built into this library", var);
  // The clustered pretest runs only in the f64 megakernel variants with
  // kVarCluster (or the wavefront kernels built with it: kWfCluster), and only
  // when the shutter lies in every time group.
  const uint32_t cl_on = (p->precision == RTW_PRECISION_F64 &&
                          (p->engine == RTW_ENGINE_MEGAKERNEL ? (var & rtwk::kVarClusterBit) != 0 : rtwk::kWfCluster))
                             ? clusters_usable(sc, cam)
                             : 0u;
  size_t lds = lds_bytes(sc, (int)p->precision, cl_on ? sc->v64.n_clusters : 0u);
  if (p->engine == RTW_ENGINE_MEGAKERNEL && (var & rtwk::kVarHomeLdsBit) != 0)
    lds += 8 + (rtwk::kHomeLdsBytesPerWave + ((var & rtwk::kVarPathLdsBit) ? rtwk::kPathLdsBytesPerWave : 0) +
                ((var & rtwk::kVarUnitBaseBit) ? rtwk::kUnitBaseLdsBytesPerWave : 0)) *
                   (rtwk::kTraceBlock / 64);  // (8: alignment of the home block)
  if (lds > 64 * 1024) return fail(RTW_UNSUPPORTED, "scene tables need %zu B of LDS", lds);
  const int bpc = blocks_per_cu(dev, (int)p->precision, lds, var);
  const int cus = device_cus(dev);
  uint32_t total_units = 0;
  hipError_t e;
  if (timer) HIP_TRY(hipEventRecord(timer->start, stream));
  if (p->engine == RTW_ENGINE_WAVEFRONT) {
    if (mode == 2) return fail(RTW_UNSUPPORTED, "phase profile runs on the megakernel engine");
    int st;
    if (p->precision == RTW_PRECISION_F32) {
      rtwk::TraceArgs<float> a;
      fill_args(a, sc->v32, cam, p, ws, L, seed_adv);
      mask_args(a);
      a.sc.n_clusters = 0u;  // f32: no clustered pretest
      st = run_wavefront<float>(a, p, ws, L, dev, lds, stream, mode == 1);
    } else {
      rtwk::TraceArgs<double> a;
      fill_args(a, sc->v64, cam, p, ws, L, seed_adv);
      mask_args(a);
      a.sc.cluster_on = cl_on;  // (0 unless the bounce kernels were built with the clustered pretest)
      if (!cl_on) a.sc.n_clusters = 0u;
      st = run_wavefront<double>(a, p, ws, L, dev, lds, stream, mode == 1);
    }
    if (st != RTW_OK) return st;
    e = hipSuccess;
  } else if (p->precision == RTW_PRECISION_F32) {
    rtwk::TraceArgs<float> a;
    fill_args(a, sc->v32, cam, p, ws, L, seed_adv);
    mask_args(a);
    a.sc.n_clusters = 0u;  // f32: no clustered pretest
    total_units = a.total_units;
    const uint32_t want = (total_units + 255) / 256;
    const uint32_t grid = std::max(1u, std::min((uint32_t)(cus * bpc), want));
    e = rtwk::launch_trace_f32(a, grid, lds, stream, mode, var);
  } else {
    rtwk::TraceArgs<double> a;
    fill_args(a, sc->v64, cam, p, ws, L, seed_adv);
    mask_args(a);
    a.sc.cluster_on = cl_on;
    if (!cl_on) a.sc.n_clusters = 0u;  // nothing to stage (lds_bytes above)
    total_units = a.total_units;
    const uint32_t want = (total_units + 255) / 256;
    const uint32_t grid = std::max(1u, std::min((uint32_t)(cus * bpc), want));
    e = rtwk::launch_trace_f64(a, grid, lds, stream, mode, var);
  }
  if (e != hipSuccess) return fail(RTW_EHIP, "trace kernel launch: %s", hipGetErrorString(e));
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
  if (validate(p) != RTW_OK) return 0;
  return ws_layout(p).total;
}

int rtw_timer_create(rtw_timer* out) {
  if (!out) return fail(RTW_EINVAL, "timer out is NULL");
  auto* t = new rtw_timer_s;
  if (hipEventCreate(&t->start) != hipSuccess || hipEventCreate(&t->stop) != hipSuccess) {
    delete t;
    return fail(RTW_EHIP, "hipEventCreate failed");
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
  if (!out) return fail(RTW_EINVAL, "probe out is NULL");
  *out = nullptr;
  if (!(wall_ms > 0.0 && wall_ms < 600e3)) return fail(RTW_EINVAL, "probe window %g ms outside (0, 600 s)", wall_ms);
  // the s_memrealtime rate of the current device (kHz), not an assumed 100 MHz
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0)
    return fail(RTW_EHIP, "probe: wall-clock rate of device %d unavailable", dev);
  auto* p = new rtw_sclk_probe_s;
  p->s = static_cast<hipStream_t>(stream);
  if (hipMalloc(reinterpret_cast<void**>(&p->d), sizeof(double)) != hipSuccess) {
    delete p;
    return fail(RTW_ENOMEM, "probe: hipMalloc failed");
  }
  hipLaunchKernelGGL(sclk_probe_kernel, dim3(1), dim3(64), 0, p->s, (unsigned long long)(wall_ms * khz),
                     (double)khz * 1e-3, p->d);
  if (hipGetLastError() != hipSuccess) {
    (void)hipFree(p->d);
    delete p;
    return fail(RTW_EHIP, "probe kernel launch failed");
  }
  *out = p;
  return RTW_OK;
}
int rtw_sclk_probe_end(rtw_sclk_probe p, double* mhz) {
  if (!p || !mhz) return fail(RTW_EINVAL, "probe/mhz is NULL");
  int st = RTW_OK;
  if (hipStreamSynchronize(p->s) != hipSuccess || hipMemcpy(mhz, p->d, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    st = fail(RTW_EHIP, "probe read failed");
  (void)hipFree(p->d);
  delete p;
  return st;
}

int rtw_timer_elapsed_ms(rtw_timer t, float* ms) {
  if (!t || !ms) return fail(RTW_EINVAL, "timer/ms is NULL");
  if (!t->recorded) return fail(RTW_EINVAL, "timer was never recorded");
  HIP_TRY(hipEventSynchronize(t->stop));
  HIP_TRY(hipEventElapsedTime(ms, t->start, t->stop));
  return RTW_OK;
}

int rtw_render_device(rtw_scene sc, const rtw_camera* cam, const rtw_params* p, void* workspace,
                      size_t ws_bytes, uint8_t* d_rgb, float* d_mean, void* stream, rtw_timer timer) {
  if (!sc || !cam) return fail(RTW_EINVAL, "scene/camera is NULL");
  if (!d_rgb) return fail(RTW_EINVAL, "d_rgb is NULL");
  const int v = validate(p);
  if (v != RTW_OK) return v;
  return launch_all(sc, cam, p, workspace, ws_bytes, d_rgb, d_mean, static_cast<hipStream_t>(stream), timer, 0);
}

// The scene's feature buffers (rtw_guides.hip).
int rtw_scene_guides_device(rtw_scene sc, const rtw_camera* cam, const rtw_params* p, rtw_guide* d_guides,
                            void* stream) {
  if (!sc) return fail(RTW_EINVAL, "rtw_scene_guides_device: scene is NULL");
  rtwk::SceneGuideArgs a;
  const int st = rtw_guide_ray_fill(a.r, "rtw_scene_guides_device", cam, p, d_guides);
  if (st != RTW_OK) return st;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != sc->device)
    return fail(RTW_EINVAL, "rtw_scene_guides_device: scene lives on device %d, current is %d", sc->device, dev);
  a.sc = sc->v64;
  const hipError_t e = rtwk::launch_scene_guides(a, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(RTW_EHIP, "guide kernel launch: %s", hipGetErrorString(e));
  return RTW_OK;
}

// The statistics pass: one render in counting mode, the kernels' 32 statistics
// words copied back (rtw_hip.h RTW_STAT_*; words 16.. are the diagnostic
// build's phase stamps).
static int stats_pass(rtw_scene sc, const rtw_camera* cam, const rtw_params* p, void* workspace, size_t ws_bytes,
               unsigned long long (&st)[32]) {
  if (!sc || !cam) return fail(RTW_EINVAL, "scene/camera is NULL");
  const int v = validate(p);
  if (v != RTW_OK) return v;
  // RTW_PHASE_PROFILE=1: diagnostic build with per-phase s_memtime stamps.
  const char* prof = dev_knob("RTW_PHASE_PROFILE");
  const int mode = (prof && prof[0] == '1') ? 2 : 1;
#ifndef RTW_MEASURE
  if (mode == 2) return fail(RTW_UNSUPPORTED, "RTW_PHASE_PROFILE needs the -DRTW_MEASURE build (tools/gpu_phase.sh)");
#endif
  const int r = launch_all(sc, cam, p, workspace, ws_bytes, nullptr, nullptr, nullptr, nullptr, mode);
  if (r != RTW_OK) return r;
  HIP_TRY(hipDeviceSynchronize());
  for (auto& x : st) x = 0;
  const WsLayout L = ws_layout(p);
  HIP_TRY(hipMemcpy(st, static_cast<unsigned char*>(workspace) + L.stats_off, sizeof(st), hipMemcpyDeviceToHost));
  if (mode == 1 && dev_knob("RTW_COUNTS_VERBOSE")) {
    fprintf(stderr, "[rtw counts] samples %llu segments %llu skipped %llu cand_wave_iters %llu cand_lanes %llu "
            "disc_ge0_lanes %llu sphere_loop_wave_iters %llu cull_survivor_lanes %llu cull_exact_wave_iters %llu "
            "cluster_wave_tests %llu cluster_wave_skips %llu\n", st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8],
            st[11], st[12]);
    if (st[13])  // wavefront engine, wf_drain
      fprintf(stderr, "[rtw counts] drain wave iterations %llu, drained segments per wave iteration %.2f of 64\n",
              st[13], (double)st[9] / (double)st[13]);
  }
  if (mode == 2) {
    const char* names[10] = {"refill",  "start_sample", "wide+pretest", "hit+kind",    "tail",
                             "loop_top", "exact_survivors", "coop_ball", "hitrec+scatter", "-"};
    unsigned long long tot = 0;
    for (int i = 0; i < 10; ++i) tot += st[16 + i];
    for (int i = 0; i < 9; ++i)
      fprintf(stderr, "[rtw phase] %-15s %6.2f%%  (%llu wave-cycles)\n", names[i], tot ? 100.0 * st[16 + i] / tot : 0.0,
              st[16 + i]);
  }
  return RTW_OK;
}

int rtw_render_stats(rtw_scene sc, const rtw_camera* cam, const rtw_params* p, void* workspace, size_t ws_bytes,
                     uint64_t stats_out[RTW_STATS_WORDS]) {
  if (!stats_out) return fail(RTW_EINVAL, "stats is NULL");
  unsigned long long st[32];
  const int r = stats_pass(sc, cam, p, workspace, ws_bytes, st);
  if (r != RTW_OK) return r;
  for (int i = 0; i < RTW_STATS_WORDS; ++i) stats_out[i] = st[i];
  return RTW_OK;
}

int rtw_render_counts_ex(rtw_scene sc, const rtw_camera* cam, const rtw_params* p, void* workspace,
                         size_t ws_bytes, uint64_t counts_out[6]) {
  if (!counts_out) return fail(RTW_EINVAL, "counts is NULL");
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
  if (!counts_out) return fail(RTW_EINVAL, "scene/camera/counts is NULL");
  uint64_t c[6];
  const int r = rtw_render_counts_ex(sc, cam, p, workspace, ws_bytes, c);
  if (r == RTW_OK)
    for (int i = 0; i < 4; ++i) counts_out[i] = c[i];
  return r;
}

int rtw_render(const rtw_camera* cam, const rtw_sphere* spheres, uint32_t n, const rtw_material* mats, uint32_t nm,
               const rtw_params* p, uint8_t* rgb_out, float* mean_out) {
  if (!cam || !rgb_out) return fail(RTW_EINVAL, "camera/rgb_out is NULL");
  const int v = validate(p);
  if (v != RTW_OK) return v;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(RTW_ENODEV, "no HIP device visible");
  int prev = 0;
  HIP_TRY(hipGetDevice(&prev));
  const int dev = p->device < 0 ? prev : p->device;
  if (dev >= ndev) return fail(RTW_EINVAL, "device %d >= device count %d", dev, ndev);
  HIP_TRY(hipSetDevice(dev));
  rtw_scene sc = nullptr;
  int st = rtw_scene_create(spheres, n, mats, nm, &sc);
  if (st != RTW_OK) {
    (void)hipSetDevice(prev);
    return st;
  }
  const size_t wsb = ws_layout(p).total;
  const size_t pix = (size_t)p->row_count * p->width * 3;
  void *ws = nullptr, *d_rgb = nullptr, *d_mean = nullptr;
  hipStream_t s = nullptr;
  st = RTW_OK;
  if (hipMalloc(&ws, wsb) != hipSuccess || hipMalloc(&d_rgb, pix) != hipSuccess ||
      (mean_out && hipMalloc(&d_mean, pix * sizeof(float)) != hipSuccess)) {
    st = fail(RTW_ENOMEM, "rtw_render: device allocation failed");
  }
  if (st == RTW_OK && hipStreamCreate(&s) != hipSuccess) st = fail(RTW_EHIP, "hipStreamCreate failed");
  if (st == RTW_OK)
    st = launch_all(sc, cam, p, ws, wsb, static_cast<uint8_t*>(d_rgb), static_cast<float*>(d_mean), s, nullptr,
                    0);
  if (st == RTW_OK && hipStreamSynchronize(s) != hipSuccess) st = fail(RTW_EHIP, "render failed on the device");
  if (st == RTW_OK && hipMemcpy(rgb_out, d_rgb, pix, hipMemcpyDeviceToHost) != hipSuccess)
    st = fail(RTW_EHIP, "copy of rgb_out failed");
  if (st == RTW_OK && mean_out &&
      hipMemcpy(mean_out, d_mean, pix * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
    st = fail(RTW_EHIP, "copy of mean_out failed");
  if (s) (void)hipStreamDestroy(s);
  if (ws) (void)hipFree(ws);
  if (d_rgb) (void)hipFree(d_rgb);
  if (d_mean) (void)hipFree(d_mean);
  rtw_scene_destroy(sc);
  (void)hipSetDevice(prev);
  return st;
}

}  // extern "C"

// ---- helpers shared with the world path (rtw_world_capi.hip) ----
int rtw_fail(int status, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return fail(status, "%s", buf);
}
int rtw_validate_params(const rtw_params* p) { return validate(p); }
const char* rtw_dev_knob(const char* name) { return dev_knob(name); }
size_t rtw_ws_total(const rtw_params* p) { return ws_layout(p).total; }
size_t rtw_ws_stats_off(const rtw_params* p) { return ws_layout(p).stats_off; }
size_t rtw_ws_counter_off(const rtw_params* p) { return ws_layout(p).counter_off; }
int rtw_device_cus(int dev) { return device_cus(dev); }
uint32_t rtw_total_units(const rtw_params* p) {
  const uint32_t tiles_x = (p->width + rtwk::kTileW - 1) / rtwk::kTileW;
  const uint32_t tiles_y = (p->row_count + rtwk::kTileH - 1) / rtwk::kTileH;
  return tiles_x * tiles_y * 64u * n_chunks(p);  // = TraceArgs::total_units (fill_args)
}
void rtw_fill_trace_args(rtwk::TraceArgs<double>& a, const rtw_camera* cam, const rtw_params* p, unsigned char* ws,
                         uint64_t seed_adv) {
  fill_args(a, rtwk::SceneView<double>{}, cam, p, ws, ws_layout(p), seed_adv);
  a.unit_order = unit_order(kWorldUnitOrder);  // the world kernel's default (fill_args)
}
int rtw_launch_finalize(const rtw_params* p, unsigned char* ws, uint8_t* d_rgb, float* d_mean, hipStream_t s) {
  const WsLayout L = ws_layout(p);
  rtwk::FinalizeArgs f;
  f.partial = reinterpret_cast<const double*>(ws + L.partial_off);
  f.rgb = d_rgb;
  f.mean = d_mean;
  f.npix = p->row_count * p->width;
  f.n_chunks = n_chunks(p);
  f.scale = 1.0 / (double)p->spp;
  const hipError_t e = rtwk::launch_finalize(f, s);
  if (e != hipSuccess) return fail(RTW_EHIP, "finalize kernel launch: %s", hipGetErrorString(e));
  return RTW_OK;
}
int rtw_timer_mark(rtw_timer t, hipStream_t s, bool start) {
  if (hipEventRecord(start ? t->start : t->stop, s) != hipSuccess) return fail(RTW_EHIP, "timer event record failed");
  if (!start) t->recorded = true;
  return RTW_OK;
}

// ------------------------------------------------------------ accumulator ----
// Progressive rendering (rtw_hip.h rtw_accum_*).  A pass over
// samples [done, done + n) is the one-shot render of params with spp = n whose
// seed_base is advanced by done * (gamma << 16): sample s of a pixel starts at
// seed_base + (pixel << 40) * gamma + s * (gamma << 16) mod 2^64
// (rtw_device.hpp start_sample_uv), so the pass's sample j is the frame's
// sample done + j.  validate() keeps spp <= 2^24, where the kernel's
// `| s` is that addition.
namespace {
constexpr uint64_t kSeedGamma = 0x9e3779b97f4a7c15ULL;  // rtw_device.hpp kGamma

// The params of a pass of n samples of the frame `p`, for sizing: n a multiple
// of the frame's chunk, or the whole frame.
bool accum_size_params(const rtw_params* p, uint32_t n, rtw_params* pp) {
  if (validate(p) != RTW_OK) return false;
  const uint32_t c = eff_chunk(p);
  if (n == 0 || n > p->spp || (n % c != 0 && n != p->spp)) {
    fail(RTW_EINVAL, "pass of %u samples: not a multiple of the chunk %u nor the frame's %u", n, c, p->spp);
    return false;
  }
  *pp = *p;
  pp->spp = n;
  return true;
}
int accum_current(rtw_accum a, const char* who) {
  if (!a) return fail(RTW_EINVAL, "%s: accumulator is NULL", who);
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != a->device)
    return fail(RTW_EINVAL, "%s: accumulator lives on device %d but the current device is %d", who, a->device, dev);
  return RTW_OK;
}

// ---- masked state ----
// The active-set update on stream s: act &= user mask (with_user), or act = (cnt == done) (from_cnt), then the
// criterion when a budget is set and anything was folded; tile masks, tile list and counts follow.
int accum_update_active(rtw_accum a, bool with_user, bool from_cnt, hipStream_t s) {
  rtwk::ActiveArgs u;
  u.act = a->act;
  u.user = with_user ? a->user : nullptr;
  u.stat = a->stat;
  u.cnt = a->cnt;
  u.tile_mask = a->tile_mask;
  u.tile_list = a->tile_list;
  u.n_active = a->n_active;
  u.W = a->p.width;
  u.rows = a->p.row_count;
  u.tiles_x = a->tiles_x;
  u.n_tiles = a->n_tiles;
  u.chunk = a->chunk;
  u.min_spp = a->min_spp;
  u.thr = a->done > 0 ? a->thr : 0.0;
  u.done = a->done;
  u.from_cnt = from_cnt ? 1u : 0u;
  // On a failed launch the host's counts stay those of the last completed update, which match the list the
  // device still holds (a tile list that is a superset of the non-empty tiles deals only units the masks refuse).
  const hipError_t e = rtwk::launch_accum_active(u, s);
  a->counts_known = false;  // (whatever ran of it: the counts are read again before they are used)
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);
    return fail(RTW_EHIP, "active-set kernel launch: %s", hipGetErrorString(e));
  }
  if (hipEventRecord(a->updated, s) != hipSuccess) {  // no event to wait for: wait here instead
    (void)hipStreamSynchronize(s);
    return fail(RTW_EHIP, "active-set update: event record failed");
  }
  return RTW_OK;
}
// Waits for the last update and reads its two counts (the per-pass readback).
int accum_wait_active(rtw_accum a) {
  if (a->counts_known) return RTW_OK;
  HIP_TRY(hipEventSynchronize(a->updated));
  HIP_TRY(hipMemcpy(a->host_active, a->n_active, sizeof(a->host_active), hipMemcpyDeviceToHost));
  a->counts_known = true;
  return RTW_OK;
}
// Enters the masked state: every pixel holds `done` samples and is active.
int accum_enter_masked(rtw_accum a) {
  if (a->masked) return RTW_OK;
  HIP_TRY(hipDeviceSynchronize());  // every enqueued pass, whichever stream it ran on
  a->tiles_x = (a->p.width + rtwk::kTileW - 1) / rtwk::kTileW;
  a->n_tiles = a->tiles_x * ((a->p.row_count + rtwk::kTileH - 1) / rtwk::kTileH);
  const size_t cnt_b = al256((size_t)a->npix * 4), act_b = al256(a->npix), mask_b = al256((size_t)a->n_tiles * 8),
               list_b = al256((size_t)a->n_tiles * 4);
  const size_t bytes = cnt_b + 2 * act_b + mask_b + list_b + 256;
  void* d = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess) return fail(RTW_ENOMEM, "masked accumulator state: hipMalloc(%zu)", bytes);
  hipEvent_t ev = nullptr;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
    (void)hipFree(d);
    return fail(RTW_EHIP, "masked accumulator state: event creation failed");
  }
  auto* b = static_cast<unsigned char*>(d);
  a->mbuf = d;
  a->cnt = reinterpret_cast<uint32_t*>(b);
  a->act = b + cnt_b;
  a->user = a->act + act_b;
  a->tile_mask = reinterpret_cast<uint64_t*>(a->user + act_b);
  a->tile_list = reinterpret_cast<uint32_t*>(b + cnt_b + 2 * act_b + mask_b);
  a->n_active = reinterpret_cast<uint32_t*>(b + cnt_b + 2 * act_b + mask_b + list_b);
  a->updated = ev;
  int st = RTW_OK;
  if (hipMemset(d, 0, bytes) != hipSuccess || hipMemset(a->act, 1, a->npix) != hipSuccess ||
      rtwk::launch_accum_fill_u32(a->cnt, a->npix, a->done, nullptr) != hipSuccess)
    st = fail(RTW_EHIP, "masked accumulator state: initialisation failed");
  if (st == RTW_OK) {
    const double thr = a->thr;  // (entering applies no criterion: the caller does, after setting its budget)
    a->thr = 0.0;
    st = accum_update_active(a, false, false, nullptr);
    a->thr = thr;
  }
  if (st == RTW_OK && hipDeviceSynchronize() != hipSuccess) st = fail(RTW_EHIP, "masked accumulator state: sync failed");
  if (st != RTW_OK) {
    (void)hipEventDestroy(ev);
    (void)hipFree(d);
    a->mbuf = nullptr, a->updated = nullptr;
    return st;
  }
  a->masked = true;
  return RTW_OK;
}
}  // namespace

bool rtw_accum_size_params(const rtw_params* p, uint32_t n, rtw_params* pp) { return accum_size_params(p, n, pp); }

// Checks a pass of pass_spp samples against the accumulator's state; *pp = its
// render params, *seed_adv = its offset into the sample streams.  Changes
// nothing.
int rtw_accum_pass_begin(rtw_accum a, uint32_t pass_spp, rtw_params* pp, uint64_t* seed_adv) {
  const int st = accum_current(a, "accumulator pass");
  if (st != RTW_OK) return st;
  if (pass_spp == 0) return fail(RTW_EINVAL, "pass_spp must be >= 1");
  if (pass_spp > a->p.spp - a->done)
    return fail(RTW_EINVAL, "pass of %u samples after %u exceeds the frame's %u", pass_spp, a->done, a->p.spp);
  if (pass_spp % a->chunk != 0 && a->done + pass_spp != a->p.spp)
    return fail(RTW_EINVAL, "pass of %u samples after %u: not a multiple of the chunk %u and not the frame's last",
                pass_spp, a->done, a->chunk);
  *pp = a->p;
  pp->spp = pass_spp;
  *seed_adv = (uint64_t)a->done * (kSeedGamma << 16);
  return RTW_OK;
}

// The fold of a rendered pass (its chunk sums are in ws), enqueued on s; the
// accumulator's sample count advances here, at enqueue time.
int rtw_accum_pass_fold(rtw_accum a, const rtw_params* pp, unsigned char* ws, hipStream_t s) {
  rtwk::FoldArgs f;
  f.partial = reinterpret_cast<const double*>(ws + ws_layout(pp).partial_off);
  f.sum = a->sum;
  f.stat = a->stat;
  f.npix = a->npix;
  f.n_chunks = n_chunks(pp);
  f.n_full = pp->spp / a->chunk;  // (a last chunk of fewer samples: into the sum only)
  if (a->masked) {  // active pixels only, then the criterion and the next pass's tile list
    rtwk::MaskedFoldArgs m;
    m.f = f;
    m.act = a->act;
    m.cnt = a->cnt;
    m.pass_spp = pp->spp;
    const hipError_t e = rtwk::launch_accum_fold_masked(m, s);
    if (e != hipSuccess) return fail(RTW_EHIP, "masked fold kernel launch: %s", hipGetErrorString(e));
    // The fold is enqueued: the sums and counts hold the pass, so `done` does from here on, whatever becomes
    // of the update below.  Should the update fail to launch, the device keeps the previous masks, list and
    // counts, which name a superset of the active pixels: a later pass stays correct (accum_update_active).
    a->done += pp->spp;
    return accum_update_active(a, false, false, s);
  }
  const hipError_t e = rtwk::launch_accum_fold(f, s);
  if (e != hipSuccess) return fail(RTW_EHIP, "fold kernel launch: %s", hipGetErrorString(e));
  a->done += pp->spp;
  return RTW_OK;
}

int rtw_accum_pass_map(rtw_accum a, const uint32_t** tile_list, const uint64_t** tile_mask, uint32_t* active_tiles) {
  *tile_list = nullptr, *tile_mask = nullptr, *active_tiles = 0;
  if (!a->masked) return RTW_OK;
  const int st = accum_wait_active(a);
  if (st != RTW_OK) return st;
  *tile_list = a->tile_list;
  *tile_mask = a->tile_mask;
  *active_tiles = a->host_active[0];
  return RTW_OK;
}

extern "C" {

int rtw_accum_create(const rtw_params* p, rtw_accum* out) {
  if (!out) return fail(RTW_EINVAL, "rtw_accum_create: out is NULL");
  *out = nullptr;
  const int v = validate(p);
  if (v != RTW_OK) return v;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  auto* a = new rtw_accum_s;
  a->device = dev;
  a->p = *p;
  a->chunk = eff_chunk(p);
  a->npix = p->row_count * p->width;
  // sub-buffers 256-B aligned (the kernels read stat as double2)
  const size_t sum_b = al256((size_t)a->npix * 24), stat_b = al256((size_t)a->npix * 16);
  const size_t bytes = sum_b + stat_b + 2 * (rtwk::kNoiseGrid + 1) * sizeof(double);  // (x2: the masked noise's pixel counts)
  void* d = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess) {
    delete a;
    return fail(RTW_ENOMEM, "rtw_accum_create: hipMalloc(%zu)", bytes);
  }
  if (hipMemset(d, 0, bytes) != hipSuccess) {
    (void)hipFree(d);
    delete a;
    return fail(RTW_EHIP, "rtw_accum_create: hipMemset failed");
  }
  a->sum = static_cast<double*>(d);
  a->stat = a->sum + sum_b / sizeof(double);
  a->noise = a->stat + stat_b / sizeof(double);
  *out = a;
  return RTW_OK;
}

int rtw_accum_destroy(rtw_accum a) {
  if (!a) return RTW_OK;
  if (a->sum) (void)hipFree(a->sum);
  if (a->mbuf) (void)hipFree(a->mbuf);
  if (a->updated) (void)hipEventDestroy(a->updated);
  delete a;
  return RTW_OK;
}

int rtw_accum_samples(rtw_accum a, uint32_t* done) {
  if (!a || !done) return fail(RTW_EINVAL, "rtw_accum_samples: accumulator/done is NULL");
  *done = a->done;
  return RTW_OK;
}

size_t rtw_accum_workspace_bytes(const rtw_params* p, uint32_t pass_spp) {
  rtw_params pp;
  if (!accum_size_params(p, pass_spp, &pp)) return 0;
  return ws_layout(&pp).total;
}

int rtw_accum_render_device(rtw_accum a, rtw_scene sc, const rtw_camera* cam, uint32_t pass_spp, void* workspace,
                            size_t ws_bytes, void* stream, rtw_timer timer) {
  if (!a || !sc || !cam) return fail(RTW_EINVAL, "accumulator/scene/camera is NULL");
  rtw_params pp;
  uint64_t adv = 0;
  const int st = rtw_accum_pass_begin(a, pass_spp, &pp, &adv);
  if (st != RTW_OK) return st;
  return launch_all(sc, cam, &pp, workspace, ws_bytes, nullptr, nullptr, static_cast<hipStream_t>(stream), timer, 0,
                    adv, a);
}

int rtw_accum_resolve_device(rtw_accum a, uint8_t* d_rgb, float* d_mean, void* stream) {
  const int st = accum_current(a, "rtw_accum_resolve_device");
  if (st != RTW_OK) return st;
  if (!d_rgb) return fail(RTW_EINVAL, "d_rgb is NULL");
  if (a->done == 0) return fail(RTW_EINVAL, "rtw_accum_resolve_device: no sample accumulated yet");
  if (a->masked) {  // each pixel by its own count
    rtwk::ResolveCntArgs r;
    r.sum = a->sum;
    r.cnt = a->cnt;
    r.rgb = d_rgb;
    r.mean = d_mean;
    r.npix = a->npix;
    const hipError_t e = rtwk::launch_accum_resolve_cnt(r, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(RTW_EHIP, "resolve kernel launch: %s", hipGetErrorString(e));
    return RTW_OK;
  }
  rtwk::ResolveArgs r;
  r.sum = a->sum;
  r.rgb = d_rgb;
  r.mean = d_mean;
  r.npix = a->npix;
  r.scale = 1.0 / (double)a->done;
  const hipError_t e = rtwk::launch_accum_resolve(r, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(RTW_EHIP, "resolve kernel launch: %s", hipGetErrorString(e));
  return RTW_OK;
}

int rtw_accum_noise(rtw_accum a, void* stream, double* noise) {
  const int st = accum_current(a, "rtw_accum_noise");
  if (st != RTW_OK) return st;
  if (!noise) return fail(RTW_EINVAL, "noise is NULL");
  if (a->masked) {  // each pixel's own m; pixels with m < 2 left out
    rtwk::NoiseCntArgs n;
    n.stat = a->stat;
    n.cnt = a->cnt;
    n.part = a->noise;
    n.npix = a->npix;
    n.chunk = a->chunk;
    auto s = static_cast<hipStream_t>(stream);
    const hipError_t e = rtwk::launch_accum_noise_cnt(n, s);
    if (e != hipSuccess) return fail(RTW_EHIP, "noise kernel launch: %s", hipGetErrorString(e));
    double out[2] = {0.0, 0.0};
    HIP_TRY(hipMemcpyAsync(&out[0], a->noise + rtwk::kNoiseGrid, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&out[1], a->noise + 2 * rtwk::kNoiseGrid + 1, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (out[1] < 1.0) return fail(RTW_EINVAL, "rtw_accum_noise: no pixel holds two full chunks, the estimate needs 2");
    *noise = out[0];
    return RTW_OK;
  }
  const uint32_t m = a->done / a->chunk;
  if (m < 2) return fail(RTW_EINVAL, "rtw_accum_noise: %u full chunks accumulated, the estimate needs 2", m);
  rtwk::NoiseArgs n;
  n.stat = a->stat;
  n.part = a->noise;
  n.npix = a->npix;
  n.m = (double)m;
  n.denom = (double)m * (double)(m - 1) * (double)a->chunk * (double)a->chunk;
  auto s = static_cast<hipStream_t>(stream);
  const hipError_t e = rtwk::launch_accum_noise(n, s);
  if (e != hipSuccess) return fail(RTW_EHIP, "noise kernel launch: %s", hipGetErrorString(e));
  HIP_TRY(hipMemcpyAsync(noise, a->noise + rtwk::kNoiseGrid, sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return RTW_OK;
}

int rtw_accum_read(rtw_accum a, double* sum_out, double* stat_out) {
  const int st = accum_current(a, "rtw_accum_read");
  if (st != RTW_OK) return st;
  if (!sum_out) return fail(RTW_EINVAL, "sum_out is NULL");
  HIP_TRY(hipDeviceSynchronize());  // every enqueued pass, whichever stream it ran on
  HIP_TRY(hipMemcpy(sum_out, a->sum, (size_t)a->npix * 24, hipMemcpyDeviceToHost));
  if (stat_out) HIP_TRY(hipMemcpy(stat_out, a->stat, (size_t)a->npix * 16, hipMemcpyDeviceToHost));
  return RTW_OK;
}

int rtw_accum_load(rtw_accum a, const double* sum, const double* stat, uint32_t samples_done) {
  const int st = accum_current(a, "rtw_accum_load");
  if (st != RTW_OK) return st;
  if (!sum || !stat) return fail(RTW_EINVAL, "sum/stat is NULL");
  if (samples_done > a->p.spp || (samples_done % a->chunk != 0 && samples_done != a->p.spp))
    return fail(RTW_EINVAL, "rtw_accum_load: %u samples is not a multiple of the chunk %u nor the frame's %u",
                samples_done, a->chunk, a->p.spp);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(a->sum, sum, (size_t)a->npix * 24, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(a->stat, stat, (size_t)a->npix * 16, hipMemcpyHostToDevice));
  a->done = samples_done;
  if (a->masked) {  // all counts = samples_done, all pixels active; then the budget's criterion, as after a fold
    if (rtwk::launch_accum_fill_u32(a->cnt, a->npix, samples_done, nullptr) != hipSuccess)
      return fail(RTW_EHIP, "rtw_accum_load: count fill failed");
    const int us = accum_update_active(a, false, true, nullptr);
    if (us != RTW_OK) return us;
    HIP_TRY(hipDeviceSynchronize());
  }
  return RTW_OK;
}

int rtw_accum_set_mask(rtw_accum a, const uint8_t* mask) {
  if (!a || !mask) return fail(RTW_EINVAL, "rtw_accum_set_mask: accumulator/mask is NULL");
  int st = accum_current(a, "rtw_accum_set_mask");
  if (st != RTW_OK) return st;
  st = accum_enter_masked(a);
  if (st != RTW_OK) return st;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(a->user, mask, a->npix, hipMemcpyHostToDevice));
  st = accum_update_active(a, true, false, nullptr);
  if (st != RTW_OK) return st;
  return accum_wait_active(a);
}

int rtw_accum_set_adaptive(rtw_accum a, double tol, uint32_t min_spp) {
  if (!a) return fail(RTW_EINVAL, "rtw_accum_set_adaptive: accumulator is NULL");
  if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(RTW_EINVAL, "rtw_accum_set_adaptive: tol must be finite and >= 0");
  int st = accum_current(a, "rtw_accum_set_adaptive");
  if (st != RTW_OK) return st;
  if (tol == 0.0) {  // no budget from here on; what has gone inactive stays so
    a->tol = a->thr = 0.0;
    a->min_spp = 0;
    return RTW_OK;
  }
  st = accum_enter_masked(a);
  if (st != RTW_OK) return st;
  a->tol = tol;
  a->thr = tol * tol;
  a->min_spp = min_spp;
  if (a->done == 0) return RTW_OK;
  HIP_TRY(hipDeviceSynchronize());
  st = accum_update_active(a, false, false, nullptr);
  if (st != RTW_OK) return st;
  return accum_wait_active(a);
}

int rtw_accum_active(rtw_accum a, uint32_t* pixels, uint32_t* tiles) {
  if (!a || !pixels || !tiles) return fail(RTW_EINVAL, "rtw_accum_active: accumulator/pixels/tiles is NULL");
  int st = accum_current(a, "rtw_accum_active");
  if (st != RTW_OK) return st;
  if (!a->masked) {
    *pixels = a->npix;
    *tiles = ((a->p.width + rtwk::kTileW - 1) / rtwk::kTileW) * ((a->p.row_count + rtwk::kTileH - 1) / rtwk::kTileH);
    return RTW_OK;
  }
  st = accum_wait_active(a);
  if (st != RTW_OK) return st;
  *tiles = a->host_active[0];
  *pixels = a->host_active[1];
  return RTW_OK;
}

int rtw_accum_read_counts(rtw_accum a, uint32_t* cnt_out) {
  if (!a || !cnt_out) return fail(RTW_EINVAL, "rtw_accum_read_counts: accumulator/cnt_out is NULL");
  const int st = accum_current(a, "rtw_accum_read_counts");
  if (st != RTW_OK) return st;
  if (!a->masked) {
    std::fill(cnt_out, cnt_out + a->npix, a->done);
    return RTW_OK;
  }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(cnt_out, a->cnt, (size_t)a->npix * 4, hipMemcpyDeviceToHost));
  return RTW_OK;
}

int rtw_accum_load_counts(rtw_accum a, const double* sum, const double* stat, const uint32_t* cnt,
                          uint32_t samples_done) {
  if (!a || !sum || !stat || !cnt) return fail(RTW_EINVAL, "rtw_accum_load_counts: accumulator/sum/stat/cnt is NULL");
  int st = accum_current(a, "rtw_accum_load_counts");
  if (st != RTW_OK) return st;
  if (samples_done > a->p.spp || (samples_done % a->chunk != 0 && samples_done != a->p.spp))
    return fail(RTW_EINVAL, "rtw_accum_load_counts: %u samples is not a multiple of the chunk %u nor the frame's %u",
                samples_done, a->chunk, a->p.spp);
  for (uint32_t i = 0; i < a->npix; ++i)
    if (cnt[i] > samples_done || (cnt[i] % a->chunk != 0 && cnt[i] != a->p.spp))
      return fail(RTW_EINVAL, "rtw_accum_load_counts: pixel %u holds %u samples: above the %u done, or off the chunk %u",
                  i, cnt[i], samples_done, a->chunk);
  st = accum_enter_masked(a);
  if (st != RTW_OK) return st;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(a->sum, sum, (size_t)a->npix * 24, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(a->stat, stat, (size_t)a->npix * 16, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(a->cnt, cnt, (size_t)a->npix * 4, hipMemcpyHostToDevice));
  a->done = samples_done;
  st = accum_update_active(a, false, true, nullptr);
  if (st != RTW_OK) return st;
  return accum_wait_active(a);
}

}  // extern "C"
