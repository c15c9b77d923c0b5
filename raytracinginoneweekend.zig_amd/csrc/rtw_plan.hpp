// rtw_plan.hpp — the render plan: everything a render derives from its
// rtw_params alone — validation, the chunk / tile / unit arithmetic, the
// wavefront engine's set and segment counts, and the layout of every device
// allocation the C ABI carves up (the workspace with its counter block and
// wavefront queue sets, the accumulator's two allocations, the world ring).
// Each is defined here once; rtw_capi.hip, rtw_wavefront_host.hip,
// rtw_accum_capi.hip and rtw_world_capi.hip take sizes and pointers from it.
// Host only, no HIP and no environment: tests/native/plan_check.cpp builds it
// with a plain C++ compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "rtw_hip.h"
#include "rtw_layout.hpp"

namespace rtwp {

// Returns RTW_OK, or the status of the first failed check with its message in `msg`.
int validate_params(const rtw_params* p, std::string& msg);

// ---- derived quantities (of validated params) ----
inline uint32_t eff_chunk(const rtw_params* p) { return std::min(p->chunk ? p->chunk : RTW_DEFAULT_CHUNK, p->spp); }
inline uint32_t n_chunks(const rtw_params* p) { return (p->spp + eff_chunk(p) - 1) / eff_chunk(p); }
inline uint32_t tiles_x(const rtw_params* p) { return (p->width + rtwk::kTileW - 1) / rtwk::kTileW; }
inline uint32_t tiles_y(const rtw_params* p) { return (p->row_count + rtwk::kTileH - 1) / rtwk::kTileH; }
inline uint32_t frame_tiles(const rtw_params* p) { return tiles_x(p) * tiles_y(p); }
// Work units of `tiles` tiles: one per pixel slot of a tile (edge tiles keep their padding slots) and chunk.
inline uint64_t tile_units(uint64_t tiles, uint32_t chunks) { return tiles * (rtwk::kTileW * rtwk::kTileH) * chunks; }
// (validate_params keeps it below 2^31: waves overshoot the 32-bit queue head by less than that)
inline uint64_t total_units(const rtw_params* p) { return tile_units(frame_tiles(p), n_chunks(p)); }

// Wavefront queue sets (params.wf_sets): the in-flight paths are split over
// independent sets (queues, home slots, segment counts, reservoirs, drain
// ring), each driven on its own HIP stream, so one set's launch ramps, tails
// and drain overlap the other sets' bounce launches.  All sets take units from
// the one device queue: a unit belongs to one slot of one set, its chunk sum
// keeps its sample order, the image keeps its bits.
constexpr uint32_t kWfMaxSets = RTW_MAX_WF_SETS;
inline uint32_t wf_sets(const rtw_params* p) { return p->wf_sets ? p->wf_sets : RTW_DEFAULT_WF_SETS; }
// The in-register drain (params.wf_drain): wf_drain (RTW_WF_DRAIN_SAMPLES,
// samples dealt to the wave's free lanes, default), wf_finish
// (RTW_WF_DRAIN_SLOTS: a lane runs its own slot's samples) or none.  Only
// wf_drain uses the drain ring, so only it reserves one.
inline bool wf_per_sample_drain(const rtw_params* p) { return p->wf_drain == RTW_WF_DRAIN_SAMPLES; }
// Segments of one queue set: its share of wf_paths rounded up to whole segments (one per wave).
uint32_t wf_segs(const rtw_params* p);

// ---- layouts ----
inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// Regions of one allocation laid end to end, each at a 256-B aligned offset.
struct Region {
  size_t off, elems, elem_size;
};
struct Regions {
  static constexpr uint32_t kMax = 40;
  Region r[kMax];
  uint32_t n = 0;
  size_t bytes = 0;  // the end of the last region
  uint32_t put(size_t elems, size_t elem_size);  // appends a region, returns its index
  size_t off(uint32_t i) const { return r[i].off; }
};

// One wavefront queue set: two path queues (rtwk::PathBuf: a region per
// member), the split form's hit arrays, the home slots, per-segment counts
// (x2), unit reservoirs and (wf_drain only) the drain ring.  The fields index
// `g.r`; drain_buf = kNone without a ring.
struct WfSetLayout {
  static constexpr uint32_t kNone = ~0u;
  Regions g;
  uint32_t queue[2];  // first region of queue A and of queue B
  uint32_t hit_t, hit_k, home, seg_a, seg_b, seg_resv, drain_buf;
};
WfSetLayout wf_set_layout(const rtw_params* p);

// Workspace: partial chunk sums | counter block | wavefront queue sets (engine 1 only).
// The counter block is zeroed before every launch: the unit queue's head, one
// live-path word per queue set (wf_count), wf_step's live_acc pair per set,
// and the 32 u64 statistics words.
struct WsLayout {
  static constexpr size_t kLiveOff = 64, kLiveAccOff = 128, kStatsOff = 256, kCounterBytes = 512;
  static_assert(kLiveOff + kWfMaxSets * 4 <= kLiveAccOff && kLiveAccOff + kWfMaxSets * 8 <= kStatsOff &&
                    kStatsOff + 32 * 8 <= kCounterBytes, "the counter block holds every set's words and pairs");
  size_t partial_off, partial_bytes;
  size_t counter_off, live_off, live_acc_off, stats_off, counter_bytes;
  size_t wf_off, wf_set_bytes, total;
};
WsLayout ws_layout(const rtw_params* p);
// The world kernel's tail rings follow the common workspace.
inline size_t world_ring_off(const rtw_params* p) { return al256(ws_layout(p).total); }

// The accumulator's main allocation (the kernels read stat as double2) ...
enum AccumRegion { kAccSum, kAccStat, kAccNoise };  // [npix][3] f64 | [npix][2] f64 | 2 x (kNoiseGrid + 1) f64
Regions accum_layout(const rtw_params* p);
// ... and its masked state's.
enum MaskedRegion { kMskCnt, kMskAct, kMskUser, kMskTileMask, kMskTileList, kMskNActive };
Regions accum_masked_layout(const rtw_params* p);

}  // namespace rtwp
