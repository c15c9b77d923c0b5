// rtw_plan.cpp — the render plan (rtw_plan.hpp): validation of rtw_params and
// the layouts sized from them.  Host only: no HIP, no environment.
#include "rtw_plan.hpp"

#include <cstdarg>
#include <cstdio>

namespace rtwp {
namespace {

int fail(std::string& msg, int status, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  msg = buf;
  return status;
}

}  // namespace

int validate_params(const rtw_params* p, std::string& msg) {
  if (!p) return fail(msg, RTW_EINVAL, "params is NULL");
  if (p->width < 2 || p->height < 2)
    return fail(msg, RTW_EINVAL, "image %ux%u: width and height must be >= 2 (main.zig:390-391 divide by W-1, H-1)",
                p->width, p->height);
  if (p->spp == 0) return fail(msg, RTW_EINVAL, "spp must be >= 1");
  if ((uint64_t)p->width * p->height > (1ull << 24))
    return fail(msg, RTW_UNSUPPORTED, "image of %llu pixels exceeds 2^24 (per-sample RNG key layout)",
                (unsigned long long)p->width * p->height);
  if (p->spp > (1u << 24)) return fail(msg, RTW_UNSUPPORTED, "spp %u exceeds 2^24", p->spp);
  if (p->row_stride == 0 || p->row_count == 0) return fail(msg, RTW_EINVAL, "row_stride and row_count must be >= 1");
  if ((uint64_t)p->row_begin + (uint64_t)(p->row_count - 1) * p->row_stride >= p->height)
    return fail(msg, RTW_EINVAL, "rows %u + k*%u (k < %u) exceed height %u", p->row_begin, p->row_stride,
                p->row_count, p->height);
  if (p->precision > RTW_PRECISION_F32) return fail(msg, RTW_EINVAL, "precision %u", p->precision);
  if (p->engine > RTW_ENGINE_WAVEFRONT) return fail(msg, RTW_EINVAL, "engine %u", p->engine);
  if (p->wf_sets > kWfMaxSets) return fail(msg, RTW_EINVAL, "wf_sets %u outside [0, %u]", p->wf_sets, kWfMaxSets);
  if (p->wf_drain > RTW_WF_DRAIN_NONE) return fail(msg, RTW_EINVAL, "wf_drain %u", p->wf_drain);
  if (p->wf_form > RTW_WF_SPLIT) return fail(msg, RTW_EINVAL, "wf_form %u", p->wf_form);
  if (p->world_waves > 4 || p->world_waves == 2)  // (compiled budgets: 1 = unconstrained, 3, 4)
    return fail(msg, RTW_EINVAL, "world_waves %u is not 0, 1, 3 or 4", p->world_waves);
  if (p->world_features > RTW_WORLD_FEATURES_ALL) return fail(msg, RTW_EINVAL, "world_features %u", p->world_features);
  if (p->world_traversal > RTW_WORLD_TRAVERSAL_LANE)
    return fail(msg, RTW_EINVAL, "world_traversal %u", p->world_traversal);
  if (p->wf_bounces > 16) return fail(msg, RTW_EINVAL, "wf_bounces %u outside [0, 16]", p->wf_bounces);
  if (p->wf_passes > 64) return fail(msg, RTW_EINVAL, "wf_passes %u outside [0, 64]", p->wf_passes);
  if (p->engine == RTW_ENGINE_WAVEFRONT && (p->wf_paths > (1u << 28) || (p->wf_paths && p->wf_paths < 64)))
    return fail(msg, RTW_EINVAL, "wf_paths %u outside [64, 2^28]", p->wf_paths);
  if (p->engine == RTW_ENGINE_WAVEFRONT && p->max_depth > 0xFFFFu)
    return fail(msg, RTW_UNSUPPORTED, "wavefront engine: max_depth %u > 65535", p->max_depth);
  const uint64_t units = total_units(p);
  // Headroom: waves overshoot the queue by < 2^31 units.  A claim of the primary-first loop (rtw_claim.hpp) is
  // at most kClaimMax = 8 batches, so a wave's claim that crosses the end adds at most 8 x 64 units.  A wave of
  // a launch without the tail goes on claiming one batch at a time past the end, but every such claim is
  // made for a lane without a unit and retires it (its unit is refused: the lane is done), so a wave makes
  // at most 64 of them.  A grid of G workgroups (4 waves each; G <= CUs x resident workgroups per CU) ends
  // the counter below units + 4 G x (8 + 64) x 64: G = 2^15 workgroups would still stay under units + 2^30.
  if (units > 0x7FFFFFFFull)
    return fail(msg, RTW_UNSUPPORTED, "%llu work units exceed the 32-bit queue; raise params.chunk",
                (unsigned long long)units);
  return RTW_OK;
}

uint32_t wf_segs(const rtw_params* p) {
  const uint32_t n = p->wf_paths ? p->wf_paths : RTW_DEFAULT_WF_PATHS;
  const uint32_t per_set = (n + wf_sets(p) - 1) / wf_sets(p);
  return std::max(1u, (per_set + rtwk::kSegCap - 1) / rtwk::kSegCap);
}

uint32_t Regions::put(size_t elems, size_t elem_size) {
  r[n] = {bytes, elems, elem_size};
  bytes += al256(elems * elem_size);
  return n++;
}

WfSetLayout wf_set_layout(const rtw_params* p) {
  const size_t segs = wf_segs(p), n = segs * rtwk::kSegCap;
  const size_t r = p->precision == RTW_PRECISION_F32 ? 4 : 8;
  WfSetLayout w;
  Regions& g = w.g;
  for (uint32_t& q : w.queue) {  // a region per rtwk::PathBuf member, in its order
    q = g.n;
    for (int i = 0; i < 10; ++i) g.put(n, r);  // ox oy oz dx dy dz tx ty tz tm
    g.put(n, 8);  // rs
    g.put(n, 4);  // slot
    g.put(n, 4);  // dsk
    g.put(n, 4);  // hk
  }
  w.hit_t = g.put(n, r);
  w.hit_k = g.put(n, 4);
  w.home = g.put(n, sizeof(rtwk::HomeRec));
  w.seg_a = g.put(segs, 4);
  w.seg_b = g.put(segs, 4);
  w.seg_resv = g.put(segs, 8);  // [next, end)
  w.drain_buf = wf_per_sample_drain(p) ? g.put(n * rtwk::kDrainWin * 3, r) : WfSetLayout::kNone;
  return w;
}

WsLayout ws_layout(const rtw_params* p) {
  WsLayout w;
  w.partial_off = 0;
  w.partial_bytes = (size_t)n_chunks(p) * p->row_count * p->width * 3 * sizeof(double);
  w.counter_off = al256(w.partial_bytes);
  w.live_off = w.counter_off + WsLayout::kLiveOff;
  w.live_acc_off = w.counter_off + WsLayout::kLiveAccOff;
  w.stats_off = w.counter_off + WsLayout::kStatsOff;
  w.counter_bytes = WsLayout::kCounterBytes;
  w.wf_off = w.counter_off + w.counter_bytes;
  w.wf_set_bytes = p->engine == RTW_ENGINE_WAVEFRONT ? wf_set_layout(p).g.bytes : 0;
  w.total = w.wf_off + wf_sets(p) * w.wf_set_bytes;
  return w;
}

Regions accum_layout(const rtw_params* p) {
  const size_t npix = (size_t)p->row_count * p->width;
  Regions g;
  g.put(npix * 3, sizeof(double));                      // kAccSum
  g.put(npix * 2, sizeof(double));                      // kAccStat
  g.put(2 * (rtwk::kNoiseGrid + 1), sizeof(double));    // kAccNoise (x2: the masked noise's pixel counts)
  return g;
}

Regions accum_masked_layout(const rtw_params* p) {
  const size_t npix = (size_t)p->row_count * p->width, tiles = frame_tiles(p);
  Regions g;
  g.put(npix, 4);   // kMskCnt
  g.put(npix, 1);   // kMskAct
  g.put(npix, 1);   // kMskUser
  g.put(tiles, 8);  // kMskTileMask
  g.put(tiles, 4);  // kMskTileList
  g.put(2, 4);      // kMskNActive {tiles, pixels}
  return g;
}

}  // namespace rtwp
