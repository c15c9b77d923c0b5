// rtw_accum_capi.hip — C ABI of the accumulator (include/rtw_hip.h
// rtw_accum_*): its two device allocations (rtw_plan.hpp accum_layout,
// accum_masked_layout), the checks and folds of a pass, the masked state and
// the readbacks.  The kernels are rtw_accum.hip's; the passes themselves are
// launched by rtw_capi.hip (scenes) and rtw_world_capi.hip (worlds).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "rtw_hip.h"
#include "rtw_capi_shared.hpp"
#include "rtw_internal.hpp"

// ------------------------------------------------------------ accumulator ----
// Progressive rendering (rtw_hip.h rtw_accum_*).  A pass over
// samples [done, done + n) is the one-shot render of params with spp = n whose
// seed_base is advanced by done * (gamma << 16): sample s of a pixel starts at
// seed_base + (pixel << 40) * gamma + s * (gamma << 16) mod 2^64
// (rtw_device.hpp start_sample_uv), so the pass's sample j is the frame's
// sample done + j.  validate_params keeps spp <= 2^24, where the kernel's
// `| s` is that addition.
namespace {
constexpr uint64_t kSeedGamma = 0x9e3779b97f4a7c15ULL;  // rtw_device.hpp kGamma

// The samples_done of a load (rtw_accum_load, rtw_accum_load_counts): full chunks, or the whole frame.
int load_check(rtw_accum a, const char* who, uint32_t samples_done) {
  if (samples_done > a->p.spp || (samples_done % a->chunk != 0 && samples_done != a->p.spp))
    return rtw_fail(RTW_EINVAL, "%s: %u samples is not a multiple of the chunk %u nor the frame's %u", who,
                    samples_done, a->chunk, a->p.spp);
  return RTW_OK;
}
int accum_current(rtw_accum a, const char* who) {
  if (!a) return rtw_fail(RTW_EINVAL, "%s: accumulator is NULL", who);
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != a->device)
    return rtw_fail(RTW_EINVAL, "%s: accumulator lives on device %d but the current device is %d", who, a->device, dev);
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
    return rtw_fail(RTW_EHIP, "active-set kernel launch: %s", hipGetErrorString(e));
  }
  if (hipEventRecord(a->updated, s) != hipSuccess) {  // no event to wait for: wait here instead
    (void)hipStreamSynchronize(s);
    return rtw_fail(RTW_EHIP, "active-set update: event record failed");
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
  a->tiles_x = rtwp::tiles_x(&a->p);
  a->n_tiles = rtwp::frame_tiles(&a->p);
  const rtwp::Regions M = rtwp::accum_masked_layout(&a->p);
  const size_t bytes = M.bytes;
  void* d = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess) return rtw_fail(RTW_ENOMEM, "masked accumulator state: hipMalloc(%zu)", bytes);
  hipEvent_t ev = nullptr;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
    (void)hipFree(d);
    return rtw_fail(RTW_EHIP, "masked accumulator state: event creation failed");
  }
  auto* b = static_cast<unsigned char*>(d);
  a->mbuf = d;
  a->cnt = reinterpret_cast<uint32_t*>(b + M.off(rtwp::kMskCnt));
  a->act = b + M.off(rtwp::kMskAct);
  a->user = b + M.off(rtwp::kMskUser);
  a->tile_mask = reinterpret_cast<uint64_t*>(b + M.off(rtwp::kMskTileMask));
  a->tile_list = reinterpret_cast<uint32_t*>(b + M.off(rtwp::kMskTileList));
  a->n_active = reinterpret_cast<uint32_t*>(b + M.off(rtwp::kMskNActive));
  a->updated = ev;
  int st = RTW_OK;
  if (hipMemset(d, 0, bytes) != hipSuccess || hipMemset(a->act, 1, a->npix) != hipSuccess ||
      rtwk::launch_accum_fill_u32(a->cnt, a->npix, a->done, nullptr) != hipSuccess)
    st = rtw_fail(RTW_EHIP, "masked accumulator state: initialisation failed");
  if (st == RTW_OK) {
    const double thr = a->thr;  // (entering applies no criterion: the caller does, after setting its budget)
    a->thr = 0.0;
    st = accum_update_active(a, false, false, nullptr);
    a->thr = thr;
  }
  if (st == RTW_OK && hipDeviceSynchronize() != hipSuccess) st = rtw_fail(RTW_EHIP, "masked accumulator state: sync failed");
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

// The params of a pass of n samples of the frame `p`, for sizing: n a multiple
// of the frame's chunk, or the whole frame.
bool rtw_accum_size_params(const rtw_params* p, uint32_t n, rtw_params* pp) {
  if (rtw_validate_params(p) != RTW_OK) return false;
  const uint32_t c = rtwp::eff_chunk(p);
  if (n == 0 || n > p->spp || (n % c != 0 && n != p->spp)) {
    rtw_fail(RTW_EINVAL, "pass of %u samples: not a multiple of the chunk %u nor the frame's %u", n, c, p->spp);
    return false;
  }
  *pp = *p;
  pp->spp = n;
  return true;
}

// Checks a pass of pass_spp samples against the accumulator's state; *pp = its
// render params, *seed_adv = its offset into the sample streams.  Changes
// nothing.
int rtw_accum_pass_begin(rtw_accum a, uint32_t pass_spp, rtw_params* pp, uint64_t* seed_adv) {
  const int st = accum_current(a, "accumulator pass");
  if (st != RTW_OK) return st;
  if (pass_spp == 0) return rtw_fail(RTW_EINVAL, "pass_spp must be >= 1");
  if (pass_spp > a->p.spp - a->done)
    return rtw_fail(RTW_EINVAL, "pass of %u samples after %u exceeds the frame's %u", pass_spp, a->done, a->p.spp);
  if (pass_spp % a->chunk != 0 && a->done + pass_spp != a->p.spp)
    return rtw_fail(RTW_EINVAL, "pass of %u samples after %u: not a multiple of the chunk %u and not the frame's last",
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
  f.partial = reinterpret_cast<const double*>(ws + rtwp::ws_layout(pp).partial_off);
  f.sum = a->sum;
  f.stat = a->stat;
  f.npix = a->npix;
  f.n_chunks = rtwp::n_chunks(pp);
  f.n_full = pp->spp / a->chunk;  // (a last chunk of fewer samples: into the sum only)
  if (a->masked) {  // active pixels only, then the criterion and the next pass's tile list
    rtwk::MaskedFoldArgs m;
    m.f = f;
    m.act = a->act;
    m.cnt = a->cnt;
    m.pass_spp = pp->spp;
    const hipError_t e = rtwk::launch_accum_fold_masked(m, s);
    if (e != hipSuccess) return rtw_fail(RTW_EHIP, "masked fold kernel launch: %s", hipGetErrorString(e));
    // The fold is enqueued: the sums and counts hold the pass, so `done` does from here on, whatever becomes
    // of the update below.  Should the update fail to launch, the device keeps the previous masks, list and
    // counts, which name a superset of the active pixels: a later pass stays correct (accum_update_active).
    a->done += pp->spp;
    return accum_update_active(a, false, false, s);
  }
  const hipError_t e = rtwk::launch_accum_fold(f, s);
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "fold kernel launch: %s", hipGetErrorString(e));
  a->done += pp->spp;
  return RTW_OK;
}

int rtw_accum_pass_map(rtw_accum a, RtwPassMap* map) {
  *map = RtwPassMap{};
  if (!a->masked) return RTW_OK;
  const int st = accum_wait_active(a);
  if (st != RTW_OK) return st;
  *map = {a->tile_list, a->tile_mask, a->host_active[0]};
  return RTW_OK;
}

extern "C" {

int rtw_accum_create(const rtw_params* p, rtw_accum* out) {
  if (!out) return rtw_fail(RTW_EINVAL, "rtw_accum_create: out is NULL");
  *out = nullptr;
  const int v = rtw_validate_params(p);
  if (v != RTW_OK) return v;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  auto* a = new rtw_accum_s;
  a->device = dev;
  a->p = *p;
  a->chunk = rtwp::eff_chunk(p);
  a->npix = p->row_count * p->width;
  const rtwp::Regions A = rtwp::accum_layout(p);
  const size_t bytes = A.bytes;
  void* d = nullptr;
  if (hipMalloc(&d, bytes) != hipSuccess) {
    delete a;
    return rtw_fail(RTW_ENOMEM, "rtw_accum_create: hipMalloc(%zu)", bytes);
  }
  if (hipMemset(d, 0, bytes) != hipSuccess) {
    (void)hipFree(d);
    delete a;
    return rtw_fail(RTW_EHIP, "rtw_accum_create: hipMemset failed");
  }
  auto* b = static_cast<unsigned char*>(d);
  a->sum = reinterpret_cast<double*>(b + A.off(rtwp::kAccSum));  // (offset 0: rtw_accum_destroy frees it)
  a->stat = reinterpret_cast<double*>(b + A.off(rtwp::kAccStat));
  a->noise = reinterpret_cast<double*>(b + A.off(rtwp::kAccNoise));
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
  if (!a || !done) return rtw_fail(RTW_EINVAL, "rtw_accum_samples: accumulator/done is NULL");
  *done = a->done;
  return RTW_OK;
}

size_t rtw_accum_workspace_bytes(const rtw_params* p, uint32_t pass_spp) {
  rtw_params pp;
  if (!rtw_accum_size_params(p, pass_spp, &pp)) return 0;
  return rtwp::ws_layout(&pp).total;
}

int rtw_accum_resolve_device(rtw_accum a, uint8_t* d_rgb, float* d_mean, void* stream) {
  const int st = accum_current(a, "rtw_accum_resolve_device");
  if (st != RTW_OK) return st;
  if (!d_rgb) return rtw_fail(RTW_EINVAL, "d_rgb is NULL");
  if (a->done == 0) return rtw_fail(RTW_EINVAL, "rtw_accum_resolve_device: no sample accumulated yet");
  if (a->masked) {  // each pixel by its own count
    rtwk::ResolveCntArgs r;
    r.sum = a->sum;
    r.cnt = a->cnt;
    r.rgb = d_rgb;
    r.mean = d_mean;
    r.npix = a->npix;
    const hipError_t e = rtwk::launch_accum_resolve_cnt(r, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return rtw_fail(RTW_EHIP, "resolve kernel launch: %s", hipGetErrorString(e));
    return RTW_OK;
  }
  rtwk::ResolveArgs r;
  r.sum = a->sum;
  r.rgb = d_rgb;
  r.mean = d_mean;
  r.npix = a->npix;
  r.scale = 1.0 / (double)a->done;
  const hipError_t e = rtwk::launch_accum_resolve(r, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "resolve kernel launch: %s", hipGetErrorString(e));
  return RTW_OK;
}

int rtw_accum_noise(rtw_accum a, void* stream, double* noise) {
  const int st = accum_current(a, "rtw_accum_noise");
  if (st != RTW_OK) return st;
  if (!noise) return rtw_fail(RTW_EINVAL, "noise is NULL");
  if (a->masked) {  // each pixel's own m; pixels with m < 2 left out
    rtwk::NoiseCntArgs n;
    n.stat = a->stat;
    n.cnt = a->cnt;
    n.part = a->noise;
    n.npix = a->npix;
    n.chunk = a->chunk;
    auto s = static_cast<hipStream_t>(stream);
    const hipError_t e = rtwk::launch_accum_noise_cnt(n, s);
    if (e != hipSuccess) return rtw_fail(RTW_EHIP, "noise kernel launch: %s", hipGetErrorString(e));
    double out[2] = {0.0, 0.0};
    HIP_TRY(hipMemcpyAsync(&out[0], a->noise + rtwk::kNoiseGrid, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&out[1], a->noise + 2 * rtwk::kNoiseGrid + 1, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (out[1] < 1.0) return rtw_fail(RTW_EINVAL, "rtw_accum_noise: no pixel holds two full chunks, the estimate needs 2");
    *noise = out[0];
    return RTW_OK;
  }
  const uint32_t m = a->done / a->chunk;
  if (m < 2) return rtw_fail(RTW_EINVAL, "rtw_accum_noise: %u full chunks accumulated, the estimate needs 2", m);
  rtwk::NoiseArgs n;
  n.stat = a->stat;
  n.part = a->noise;
  n.npix = a->npix;
  n.m = (double)m;
  n.denom = (double)m * (double)(m - 1) * (double)a->chunk * (double)a->chunk;
  auto s = static_cast<hipStream_t>(stream);
  const hipError_t e = rtwk::launch_accum_noise(n, s);
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "noise kernel launch: %s", hipGetErrorString(e));
  HIP_TRY(hipMemcpyAsync(noise, a->noise + rtwk::kNoiseGrid, sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return RTW_OK;
}

int rtw_accum_read(rtw_accum a, double* sum_out, double* stat_out) {
  const int st = accum_current(a, "rtw_accum_read");
  if (st != RTW_OK) return st;
  if (!sum_out) return rtw_fail(RTW_EINVAL, "sum_out is NULL");
  HIP_TRY(hipDeviceSynchronize());  // every enqueued pass, whichever stream it ran on
  HIP_TRY(hipMemcpy(sum_out, a->sum, (size_t)a->npix * 24, hipMemcpyDeviceToHost));
  if (stat_out) HIP_TRY(hipMemcpy(stat_out, a->stat, (size_t)a->npix * 16, hipMemcpyDeviceToHost));
  return RTW_OK;
}

int rtw_accum_load(rtw_accum a, const double* sum, const double* stat, uint32_t samples_done) {
  int st = accum_current(a, "rtw_accum_load");
  if (st != RTW_OK) return st;
  if (!sum || !stat) return rtw_fail(RTW_EINVAL, "sum/stat is NULL");
  st = load_check(a, "rtw_accum_load", samples_done);
  if (st != RTW_OK) return st;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(a->sum, sum, (size_t)a->npix * 24, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(a->stat, stat, (size_t)a->npix * 16, hipMemcpyHostToDevice));
  a->done = samples_done;
  if (a->masked) {  // all counts = samples_done, all pixels active; then the budget's criterion, as after a fold
    if (rtwk::launch_accum_fill_u32(a->cnt, a->npix, samples_done, nullptr) != hipSuccess)
      return rtw_fail(RTW_EHIP, "rtw_accum_load: count fill failed");
    const int us = accum_update_active(a, false, true, nullptr);
    if (us != RTW_OK) return us;
    HIP_TRY(hipDeviceSynchronize());
  }
  return RTW_OK;
}

int rtw_accum_set_mask(rtw_accum a, const uint8_t* mask) {
  if (!a || !mask) return rtw_fail(RTW_EINVAL, "rtw_accum_set_mask: accumulator/mask is NULL");
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
  if (!a) return rtw_fail(RTW_EINVAL, "rtw_accum_set_adaptive: accumulator is NULL");
  if (!(tol >= 0.0) || !std::isfinite(tol)) return rtw_fail(RTW_EINVAL, "rtw_accum_set_adaptive: tol must be finite and >= 0");
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
  if (!a || !pixels || !tiles) return rtw_fail(RTW_EINVAL, "rtw_accum_active: accumulator/pixels/tiles is NULL");
  int st = accum_current(a, "rtw_accum_active");
  if (st != RTW_OK) return st;
  if (!a->masked) {
    *pixels = a->npix;
    *tiles = rtwp::frame_tiles(&a->p);
    return RTW_OK;
  }
  st = accum_wait_active(a);
  if (st != RTW_OK) return st;
  *tiles = a->host_active[0];
  *pixels = a->host_active[1];
  return RTW_OK;
}

int rtw_accum_read_counts(rtw_accum a, uint32_t* cnt_out) {
  if (!a || !cnt_out) return rtw_fail(RTW_EINVAL, "rtw_accum_read_counts: accumulator/cnt_out is NULL");
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
  if (!a || !sum || !stat || !cnt) return rtw_fail(RTW_EINVAL, "rtw_accum_load_counts: accumulator/sum/stat/cnt is NULL");
  int st = accum_current(a, "rtw_accum_load_counts");
  if (st != RTW_OK) return st;
  st = load_check(a, "rtw_accum_load_counts", samples_done);
  if (st != RTW_OK) return st;
  for (uint32_t i = 0; i < a->npix; ++i)
    if (cnt[i] > samples_done || (cnt[i] % a->chunk != 0 && cnt[i] != a->p.spp))
      return rtw_fail(RTW_EINVAL, "rtw_accum_load_counts: pixel %u holds %u samples: above the %u done, or off the chunk %u",
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
