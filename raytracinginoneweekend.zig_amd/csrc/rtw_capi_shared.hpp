// rtw_capi_shared.hpp — what the two files of the C ABI share (rtw_capi.hip
// defines it all, rtw_world_capi.hip uses it): the handles a world render
// passes on, and the helpers of validation, workspace layout and launches.
// Internal to the library; nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>

#include "rtw_hip.h"
#include "rtw_internal.hpp"

struct rtw_timer_s {
  hipEvent_t start = nullptr, stop = nullptr;
  bool recorded = false;
};

// A frame accumulated over sample passes (rtw_hip.h rtw_accum_*).  One device
// allocation: sum [npix][3] f64 | stat [npix][2] f64 (npix * 40 B) | the noise
// reduction's kNoiseGrid + 1 words.
struct rtw_accum_s {
  int device = 0;
  rtw_params p{};      // the frame's params, copied at creation (spp = the total)
  uint32_t chunk = 0;  // the one-shot's effective chunk for p
  uint32_t done = 0;   // samples folded: a multiple of chunk, or p.spp (host state, advanced at enqueue)
  uint32_t npix = 0;
  double *sum = nullptr, *stat = nullptr, *noise = nullptr;
  // Masked state, entered by the first rtw_accum_set_mask / set_adaptive / load_counts and
  // never left: a second allocation `mbuf` with cnt [npix] u32 | act [npix] u8 | user [npix] u8 (the staged
  // mask of set_mask) | tile_mask [n_tiles] u64 | tile_list [n_tiles] u32 | n_active {tiles, pixels}.
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
int rtw_validate_params(const rtw_params* p);
const char* rtw_dev_knob(const char* name);  // environment, -DRTW_MEASURE builds only
// workspace layout (rtw_capi.hip WsLayout)
size_t rtw_ws_total(const rtw_params* p);
size_t rtw_ws_stats_off(const rtw_params* p);
size_t rtw_ws_counter_off(const rtw_params* p);
int rtw_device_cus(int dev);
uint32_t rtw_total_units(const rtw_params* p);
// the world kernel's TraceArgs (no scene view; its own unit order)
void rtw_fill_trace_args(rtwk::TraceArgs<double>& a, const rtw_camera* cam, const rtw_params* p, unsigned char* ws,
                         uint64_t seed_adv);
int rtw_launch_finalize(const rtw_params* p, unsigned char* ws, uint8_t* d_rgb, float* d_mean, hipStream_t s);
int rtw_timer_mark(rtw_timer t, hipStream_t s, bool start);
// feature buffers (rtw_guides.hip): checks the arguments of a guide entry and fills the feature ray
int rtw_guide_ray_fill(rtwk::GuideRay& g, const char* who, const rtw_camera* cam, const rtw_params* p, void* d_guides);
// accumulator passes
bool rtw_accum_size_params(const rtw_params* p, uint32_t n, rtw_params* pp);
int rtw_accum_pass_begin(rtw_accum a, uint32_t pass_spp, rtw_params* pp, uint64_t* seed_adv);
int rtw_accum_pass_fold(rtw_accum a, const rtw_params* pp, unsigned char* ws, hipStream_t s);
// The take's map for a pass of `a`: both null for a never-masked accumulator; else the device tile list and
// masks and the active tile count, after waiting for the previous active-set update (one 8-byte readback).
int rtw_accum_pass_map(rtw_accum a, const uint32_t** tile_list, const uint64_t** tile_mask, uint32_t* active_tiles);
