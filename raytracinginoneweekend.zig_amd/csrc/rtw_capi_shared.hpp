// rtw_capi_shared.hpp — what the files of the C ABI share: rtw_capi.hip
// (error state, device info, scenes, the cover-scene launches),
// rtw_wavefront_host.hip (the wavefront engine's host driver),
// rtw_accum_capi.hip (the accumulator) and rtw_world_capi.hip (general
// worlds).  The handles they pass on, the helpers of validation and launches,
// and the holders of host resources.  Sizes and layouts: rtw_plan.hpp.
// Internal to the library; nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>

#include "rtw_hip.h"
#include "rtw_internal.hpp"
#include "rtw_plan.hpp"
#include "rtw_query_plan.hpp"

struct rtw_timer_s {
  hipEvent_t start = nullptr, stop = nullptr;
  bool recorded = false;
};

// A frame accumulated over sample passes (rtw_hip.h rtw_accum_*).  One device
// allocation, rtwp::accum_layout: sum [npix][3] f64 | stat [npix][2] f64 | the
// noise reductions' words.
struct rtw_accum_s {
  int device = 0;
  rtw_params p{};      // the frame's params, copied at creation (spp = the total)
  uint32_t chunk = 0;  // the one-shot's effective chunk for p
  uint32_t done = 0;   // samples folded: a multiple of chunk, or p.spp (host state, advanced at enqueue)
  uint32_t npix = 0;
  double *sum = nullptr, *stat = nullptr, *noise = nullptr;
  // Masked state, entered by the first rtw_accum_set_mask / set_adaptive / load_counts and
  // never left: a second allocation `mbuf`, rtwp::accum_masked_layout: cnt [npix] u32 | act [npix] u8 |
  // user [npix] u8 (the staged mask of set_mask) | tile_mask [n_tiles] u64 | tile_list [n_tiles] u32 |
  // n_active {tiles, pixels}.
  bool masked = false;
  void* mbuf = nullptr;
  uint32_t* cnt = nullptr;
  uint8_t *act = nullptr, *user = nullptr;
  uint64_t* tile_mask = nullptr;
  uint32_t *tile_list = nullptr, *n_active = nullptr;
  uint32_t tiles_x = 0, n_tiles = 0;
  double tol = 0.0, thr = 0.0;   // the budget: thr = tol * tol, 0 = none
  uint32_t min_spp = 0;
  hipEvent_t updated = nullptr;  // recorded after the last active-set update
  bool counts_known = false;     // host_active holds that update's counts
  uint32_t host_active[2] = {0, 0};  // {active tiles, active pixels}
};

int rtw_fail(int status, const char* fmt, ...);  // sets rtw_last_error, returns status
#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return rtw_fail(RTW_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
int rtw_validate_params(const rtw_params* p);    // rtwp::validate_params, its message as the last error
const char* rtw_dev_knob(const char* name);      // environment, -DRTW_MEASURE builds only
int rtw_device_cus(int dev);
// resident workgroups per CU of a wavefront bounce kernel (rtwk::wf_blocks_per_cu, cached per device)
int rtw_wf_blocks_per_cu(int dev, int prec, int kernel, size_t lds);

// An event without timing, destroyed with its holder.
struct RtwEvent {
  hipEvent_t e = nullptr;
  RtwEvent() = default;
  RtwEvent(const RtwEvent&) = delete;
  RtwEvent& operator=(const RtwEvent&) = delete;
  ~RtwEvent() {
    if (e) (void)hipEventDestroy(e);
  }
  bool create() { return hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess; }
};

// The take's map of a masked accumulator's pass (TraceArgs::tile_list): the launch deals the active tiles only.
// list is null in every other render.
struct RtwPassMap {
  const uint32_t* list = nullptr;
  const uint64_t* mask = nullptr;
  uint32_t tiles = 0;
  template <typename R>
  void apply(rtwk::TraceArgs<R>& a) const {
    if (!list) return;
    a.tile_list = list;
    a.tile_mask = mask;
    a.total_units = (uint32_t)rtwp::tile_units(tiles, a.n_chunks);
  }
};
// What every render does before its launches, on `stream`: checks the workspace against L and the current
// device (*dev) against the scene's or world's (mismatch_fmt: its message, of both device numbers), takes the
// pass map of `acc` (may be null) and zeroes the counter block.  *launch = false for a pass of a masked
// accumulator with no active tile: nothing is to be launched, and the timer holds no interval.
int rtw_launch_begin(const rtwp::WsLayout& L, void* ws, size_t ws_bytes, int owner_device, const char* mismatch_fmt,
                     rtw_accum acc, rtw_timer timer, hipStream_t stream, int* dev, RtwPassMap* map, bool* launch);

// The device state of a one-shot render (rtw_render, rtw_world_render): the switch to params.device and back,
// the workspace and the two output buffers, the copies to the host.  The destructor frees and restores.
struct RtwOneShot {
  int prev = -1;  // the device to return to
  void* ws = nullptr;
  uint8_t* d_rgb = nullptr;
  float* d_mean = nullptr;
  size_t ws_bytes = 0, pix = 0;  // pix: values of an output buffer
  RtwOneShot() = default;
  RtwOneShot(const RtwOneShot&) = delete;
  RtwOneShot& operator=(const RtwOneShot&) = delete;
  ~RtwOneShot();
  int enter(const rtw_params* p);  // makes params.device current
  int alloc(const char* who, size_t workspace_bytes, const rtw_params* p, bool mean);
  int copy_back(uint8_t* rgb_out, float* mean_out) const;  // (after the caller's synchronisation)
};

// the world kernel's TraceArgs (no scene view; its own unit order)
void rtw_fill_trace_args(rtwk::TraceArgs<double>& a, const rtw_camera* cam, const rtw_params* p, unsigned char* ws,
                         uint64_t seed_adv);
int rtw_launch_finalize(const rtw_params* p, unsigned char* ws, uint8_t* d_rgb, float* d_mean, hipStream_t s);
int rtw_timer_mark(rtw_timer t, hipStream_t s, bool start);
// The wavefront engine's render of `ta` into the chunk sums (rtw_wavefront_host.hip; R = double, float).
template <typename R>
int rtw_run_wavefront(const rtwk::TraceArgs<R>& ta, const rtw_params* p, unsigned char* ws, const rtwp::WsLayout& L,
                      int dev, size_t lds, hipStream_t stream, bool stats);
// feature buffers (rtw_guides.hip): checks the arguments of a guide entry and fills the feature ray
int rtw_guide_ray_fill(rtwk::GuideRay& g, const char* who, const rtw_camera* cam, const rtw_params* p, void* d_guides);
// The device tables of an uploaded world (rtw_world_capi.hip), for entries in other files: RTW_EINVAL when the
// world is NULL or lives on another device than the current one.  feat (optional): the features the world uses
// (rtw_world.hip kFeat*), which pick a kernel's instantiation.  rtw_scene_view: the same for a scene's f64 tables.
int rtw_world_view(rtw_world w, const char* who, rtwk::WorldView* view, uint32_t* feat = nullptr);
int rtw_scene_view(rtw_scene sc, const char* who, rtwk::SceneView<double>* view);
// accumulator passes (rtw_accum_capi.hip)
bool rtw_accum_size_params(const rtw_params* p, uint32_t n, rtw_params* pp);
int rtw_accum_pass_begin(rtw_accum a, uint32_t pass_spp, rtw_params* pp, uint64_t* seed_adv);
int rtw_accum_pass_fold(rtw_accum a, const rtw_params* pp, unsigned char* ws, hipStream_t s);
// The take's map for a pass of `a`: empty for a never-masked accumulator; else the device tile list and
// masks and the active tile count, after waiting for the previous active-set update (one 8-byte readback).
int rtw_accum_pass_map(rtw_accum a, RtwPassMap* map);

// The device buffers of a host-form ray query (rtw_world_trace, rtw_scene_trace): the rays up, the records back
// after waiting for the device.  The destructor frees.
struct RtwQueryBuffers {
  rtw_ray* d_rays = nullptr;
  rtw_hit* d_hits = nullptr;
  RtwQueryBuffers() = default;
  RtwQueryBuffers(const RtwQueryBuffers&) = delete;
  RtwQueryBuffers& operator=(const RtwQueryBuffers&) = delete;
  ~RtwQueryBuffers() {
    if (d_rays) (void)hipFree(d_rays);
    if (d_hits) (void)hipFree(d_hits);
  }
  int upload(const char* who, const rtw_ray* rays, uint64_t n) {
    if (hipMalloc(reinterpret_cast<void**>(&d_rays), n * sizeof(rtw_ray)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&d_hits), n * sizeof(rtw_hit)) != hipSuccess)
      return rtw_fail(RTW_ENOMEM, "%s: device buffers for %llu rays", who, (unsigned long long)n);
    if (hipMemcpy(d_rays, rays, n * sizeof(rtw_ray), hipMemcpyHostToDevice) != hipSuccess)
      return rtw_fail(RTW_EHIP, "%s: copy of the rays failed", who);
    return RTW_OK;
  }
  int download(const char* who, rtw_hit* hits_out, uint64_t n) {
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(hits_out, d_hits, n * sizeof(rtw_hit), hipMemcpyDeviceToHost) != hipSuccess)
      return rtw_fail(RTW_EHIP, "%s: the query failed on the device", who);
    return RTW_OK;
  }
};
