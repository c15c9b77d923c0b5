// rtw_wavefront_host.hip — the host driver of the wavefront engine
// (rtw_wavefront.hip has the kernels, rtw_plan.hpp the queue sets' layout).
// Per queue set, generate, then batches of bounce launches; after each batch
// wf_count sums the segment counts of the set's queue A and the total is
// copied to pinned memory (the fused form's wf_step publishes it itself).  The
// host stops a set once a batch (checked one batch behind, so the GPU never
// idles on the poll) left its queue empty, or hands the set's drain to
// wf_drain / wf_finish once its live count shows retiring slots.  Empty
// batches cost only the launches: every wave reads its count first.  Sets run
// on their own streams, forked from and joined back to the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>

#include "rtw_capi_shared.hpp"

namespace {

using rtwp::kWfMaxSets;
using Clock = std::chrono::steady_clock;

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

constexpr uint32_t kWfBatch = 64;
constexpr int kWfIters = 8;  // even: each batch ends with the live paths in queue A

// The launch configuration of a wavefront render: the same for every set and batch of the frame.
struct WfConfig {
  uint32_t segs, nsets;
  size_t n;  // slots of one set
  bool per_sample, fused, publish, poll_check, stats;
  uint32_t refill, bounces, passes;
  int iters;  // launches per batch
  uint32_t max_grid, grid, grid_ext, grid_step;
  uint64_t max_batches;
  double timeout_s, fin_frac;
  size_t lds;
  hipStream_t stream;  // the caller's
  uint32_t *poll, *poll_dev;
};

// Development knobs (-DRTW_MEASURE builds): a count >= 1, a real number, a switch.
uint32_t knob_count(const char* name, uint32_t dflt) {
  const char* v = rtw_dev_knob(name);
  return (v && *v) ? (uint32_t)std::max(1, atoi(v)) : dflt;
}
double knob_real(const char* name, double dflt) {
  const char* v = rtw_dev_knob(name);
  return (v && *v) ? atof(v) : dflt;
}
bool knob_on(const char* name) {
  const char* v = rtw_dev_knob(name);
  return v && *v == '1';
}

template <typename R>
int wf_config(WfConfig& c, const rtwk::TraceArgs<R>& ta, const rtw_params* p, int dev, size_t lds, hipStream_t stream,
              bool stats) {
  c.segs = rtwp::wf_segs(p), c.nsets = rtwp::wf_sets(p);
  c.n = (size_t)c.segs * rtwk::kSegCap;
  c.per_sample = rtwp::wf_per_sample_drain(p);
  c.stats = stats, c.lds = lds, c.stream = stream;
  // Units per reservoir refill (kWfBatch; development knob RTW_WF_BATCH): the
  // refills' atomics against the work a reservoir still holds when the queue
  // runs dry.
  c.refill = knob_count("RTW_WF_BATCH", kWfBatch);
  // Bounce segments per path per wf_step launch (params.wf_bounces, 0 = 1):
  // the path stays in registers between them.
  c.bounces = p->wf_bounces ? p->wf_bounces : 1u;
  // Persistent grids: every resident wave slot of each bounce kernel (at most
  // one wave per segment); the same grids for every launch of the frame.
  // The drains always run max_grid = ceil(segs / waves per block) blocks: one
  // wave per segment (wf_drain has no segment loop; grid_of never sizes them).
  c.max_grid = (c.segs + rtwk::kTraceBlock / 64 - 1) / (rtwk::kTraceBlock / 64);
  // RTW_WF_GRID (development knob): N > 0 = N x the resident grid, capped at one wave per segment.
  // RTW_WF_SET_GRID (development knob): each set's bounce grid = the resident grid / N.
  const uint32_t gmul = knob_count("RTW_WF_GRID", 1u), gdiv = knob_count("RTW_WF_SET_GRID", 1u);
  auto grid_of = [&](int kernel) {
    const uint32_t per_cu = (uint32_t)rtw_wf_blocks_per_cu(dev, (int)(sizeof(R) == 4), kernel, lds);
    return std::max(1u, std::min((uint32_t)rtw_device_cus(dev) * per_cu * gmul / gdiv, c.max_grid));
  };
  c.grid = grid_of(2), c.grid_ext = grid_of(1), c.grid_step = grid_of(3);
  // Fused engine (default; params.wf_form RTW_WF_SPLIT: separate extend and
  // shade kernels): one kernel per bounce, the closest hit computed where the
  // ray is made.
  c.fused = p->wf_form == RTW_WF_FUSED;
  // Queue passes per wf_step launch (params.wf_passes, fused form): each pass
  // moves every path through the queues; a batch holds >= kWfIters passes.
  c.passes = !c.fused ? 1u : p->wf_passes ? p->wf_passes : RTW_DEFAULT_WF_PASSES;
  c.iters = std::max(2, (kWfIters / (int)c.passes) & ~1);  // even: the batch ends with the paths in queue A
  c.poll = poll_words();
  if (!c.poll) return rtw_fail(RTW_EHIP, "hipHostMalloc of the poll words failed");
  c.poll_dev = poll_words_dev(c.poll);
  if (!c.poll_dev) return rtw_fail(RTW_EHIP, "hipHostGetDevicePointer of the poll words failed");
  // development knobs: RTW_WF_POLL_KERNEL=1 polls the fused engine through
  // wf_count + copy as the split form does; RTW_WF_POLL_CHECK=1 runs both and
  // reports on stderr a batch whose published count differs from wf_count's
  c.poll_check = c.fused && knob_on("RTW_WF_POLL_CHECK");
  c.publish = c.fused && !knob_on("RTW_WF_POLL_KERNEL");
  if (c.publish && c.grid_step >= (1u << 20))
    return rtw_fail(RTW_EINVAL, "wf_step grid %u exceeds the poll ticket's 20 bits", c.grid_step);
  // Termination bound (never reached by a correct kernel): every iteration
  // advances every live path by one segment.
  c.max_batches =
      (uint64_t)ta.total_units * ta.chunk * (ta.max_depth + 1ull) / (uint64_t)(c.iters * c.passes) + 4;
  // Wall-clock guard as well (300 s; development knob RTW_WF_TIMEOUT_S): a
  // queue that never drains is reported instead of hanging the caller.
  c.timeout_s = knob_real("RTW_WF_TIMEOUT_S", 300.0);
  // Drain in registers once a set's polled live count falls below fin_frac x
  // its slots: 1 as soon as slots start to retire, i.e. the unit queue ran
  // dry; 0 with RTW_WF_DRAIN_NONE (through the queues to the end); the
  // development knob RTW_WF_FINISH sets another fraction.
  c.fin_frac = p->wf_drain == RTW_WF_DRAIN_NONE ? 0.0 : knob_real("RTW_WF_FINISH", 1.0);
  return RTW_OK;
}

// One queue set of the wavefront engine: its region of the workspace, its
// stream and its host-side progress.
template <typename R>
struct WfSet {
  rtwk::WfArgs<R> a;
  rtwk::PathBuf<R> qa, qb;
  uint32_t *seg_a = nullptr, *seg_b = nullptr;
  hipStream_t s = nullptr;
  RtwEvent ev[2];  // a batch's end, by its parity; at the end [0] the drained-state check, [1] the join
  uint64_t batch = 0;
  bool done = false;
  bool started = false;  // its generate kernel was enqueued
};

// A path queue at its regions of the set at `b`: PathBuf's members are the queue's regions, in order.
template <typename R>
rtwk::PathBuf<R> queue_at(unsigned char* b, const rtwp::WfSetLayout& W, uint32_t first) {
  static_assert(std::is_trivially_copyable<rtwk::PathBuf<R>>::value, "PathBuf is a struct of pointers");
  void* m[sizeof(rtwk::PathBuf<R>) / sizeof(void*)];
  for (size_t i = 0; i < sizeof(m) / sizeof(m[0]); ++i) m[i] = b + W.g.off(first + (uint32_t)i);
  rtwk::PathBuf<R> q;
  std::memcpy(&q, m, sizeof(q));
  return q;
}

// Set k's arguments over its region of the workspace, its stream and events; then generate -> queue A.
template <typename R>
int wf_set_up(WfSet<R>& S, uint32_t k, const WfConfig& c, const rtwk::TraceArgs<R>& ta, unsigned char* ws,
              const rtwp::WsLayout& L, const rtwp::WfSetLayout& W, int dev, hipEvent_t fork) {
  rtwk::WfArgs<R>& a = S.a;
  std::memset(&a, 0, sizeof(a));
  a.t = ta;
  unsigned char* b = ws + L.wf_off + k * L.wf_set_bytes;
  S.qa = queue_at<R>(b, W, W.queue[0]);
  S.qb = queue_at<R>(b, W, W.queue[1]);
  a.hit_t = reinterpret_cast<R*>(b + W.g.off(W.hit_t));
  a.hit_k = reinterpret_cast<int32_t*>(b + W.g.off(W.hit_k));
  a.home = reinterpret_cast<rtwk::HomeRec*>(b + W.g.off(W.home));
  S.seg_a = reinterpret_cast<uint32_t*>(b + W.g.off(W.seg_a));
  S.seg_b = reinterpret_cast<uint32_t*>(b + W.g.off(W.seg_b));
  a.seg_resv = reinterpret_cast<uint32_t*>(b + W.g.off(W.seg_resv));
  a.drain_buf = c.per_sample ? reinterpret_cast<R*>(b + W.g.off(W.drain_buf)) : nullptr;
  a.live = reinterpret_cast<uint32_t*>(ws + L.live_off) + k;
  a.n_slots = (uint32_t)c.n;
  a.n_segs = c.segs;
  a.batch = c.refill;
  a.bounces = c.bounces;
  a.passes = c.passes;
  a.hit_form = c.fused ? 1u : 0u;  // fused: queued paths carry their hit (hk, o = the hit point)
  a.live_acc = reinterpret_cast<uint32_t*>(ws + L.live_acc_off) + 2 * k;  // (zeroed with the queue head)
  a.poll_out = nullptr;  // (set per batch)
  S.s = k == 0 ? c.stream : wf_side_stream(dev, k);  // (set 0: the caller's stream, NULL = the default stream)
  if (k > 0 && !S.s) return rtw_fail(RTW_EHIP, "wavefront side stream creation failed");
  bool ev_ok = true;
  for (auto& x : S.ev) ev_ok = x.create() && ev_ok;
  if (!ev_ok) return rtw_fail(RTW_EHIP, "hipEventCreate failed");
  if (k > 0 && hipStreamWaitEvent(S.s, fork, 0) != hipSuccess) return rtw_fail(RTW_EHIP, "wavefront fork wait failed");
  a.out = S.qa;
  a.seg_out = S.seg_a;
  const hipError_t e = c.fused ? rtwk::launch_wf_generate_hit(a, c.grid_step, c.lds, S.s)
                               : rtwk::launch_wf_generate(a, c.grid, 0, S.s);
  S.started = true;
  return e == hipSuccess ? RTW_OK : rtw_fail(RTW_EHIP, "wavefront generate launch: %s", hipGetErrorString(e));
}

// One batch on set k: its bounce launches, the poll of the queue length it leaves, the batch's event.
template <typename R>
int wf_enqueue_batch(WfSet<R>& S, uint32_t k, const WfConfig& c) {
  rtwk::WfArgs<R>& a = S.a;
  hipError_t e = hipSuccess;
  // fused: the batch's wf_step launches publish the live count into this
  // batch's pinned word themselves (wf_step publish_live); split: wf_count + copy
  a.poll_out = c.publish ? c.poll_dev + 2 * k + (S.batch & 1) : nullptr;
  for (int i = 0; i < c.iters && e == hipSuccess; ++i) {
    const bool even = (i & 1) == 0 || (c.passes & 1u) == 0u;  // (an even pass count returns to its input queue)
    a.in = even ? S.qa : S.qb;
    a.out = even ? S.qb : S.qa;
    a.seg_in = even ? S.seg_a : S.seg_b;
    a.seg_out = even ? S.seg_b : S.seg_a;
    if (c.fused)
      e = rtwk::launch_wf_step(a, c.grid_step, c.lds, S.s, c.stats);
    else if ((e = rtwk::launch_wf_extend(a, c.grid_ext, c.lds, S.s)) == hipSuccess)
      e = rtwk::launch_wf_shade(a, c.grid, c.lds, S.s, c.stats);
  }
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "wavefront bounce launch: %s", hipGetErrorString(e));
  uint32_t* pw = c.poll + (c.publish ? 2 * kWfMaxSets : 0u) + 2 * k + (S.batch & 1);
  int st = RTW_OK;
  if (((!c.publish || c.poll_check) && (rtwk::launch_wf_count(S.seg_a, c.segs, a.live, S.s) != hipSuccess ||
                                        hipMemcpyAsync(pw, a.live, 4, hipMemcpyDeviceToHost, S.s) != hipSuccess)) ||
      hipEventRecord(S.ev[S.batch & 1].e, S.s) != hipSuccess)
    st = rtw_fail(RTW_EHIP, "wavefront poll enqueue failed");
  a.poll_out = nullptr;  // (the drains and checks below do not publish)
  return st;
}

// Looks at the batch before the one just enqueued on set k (so its stream holds a batch while the host waits):
// hands the set to its drain or ends it (--left) by the live count, or reports a queue that does not drain.
template <typename R>
int wf_examine_batch(WfSet<R>& S, uint32_t k, const WfConfig& c, Clock::time_point t_start, uint32_t& left) {
  const uint64_t b = S.batch++;
  if (b == 0) return RTW_OK;
  if (hipEventSynchronize(S.ev[(b - 1) & 1].e) != hipSuccess)
    return rtw_fail(RTW_EHIP, "wavefront batch failed on the device");
  const uint32_t live = c.poll[2 * k + ((b - 1) & 1)];
  if (c.poll_check && c.publish && live != c.poll[2 * kWfMaxSets + 2 * k + ((b - 1) & 1)])
    std::fprintf(stderr, "[rtw wf poll] set %u batch %llu: published %u, wf_count %u\n", k,
                 (unsigned long long)(b - 1), live, c.poll[2 * kWfMaxSets + 2 * k + ((b - 1) & 1)]);
  int st = RTW_OK;
  if (live != 0u && (double)live < c.fin_frac * (double)c.n) {  // queue A holds the paths after this batch
    rtwk::WfArgs<R>& a = S.a;
    a.in = S.qa;
    a.seg_in = S.seg_a;
    const hipError_t e = c.per_sample ? rtwk::launch_wf_drain(a, c.max_grid, c.lds, S.s, c.stats)
                                      : rtwk::launch_wf_finish(a, c.max_grid, c.lds, S.s, c.stats);
    if (e != hipSuccess) st = rtw_fail(RTW_EHIP, "wavefront finish launch: %s", hipGetErrorString(e));
  }
  if (live == 0u || (double)live < c.fin_frac * (double)c.n) {
    S.done = true;
    --left;
  } else if (b > c.max_batches || std::chrono::duration<double>(Clock::now() - t_start).count() > c.timeout_s) {
    st = rtw_fail(RTW_EHIP, "wavefront queue did not drain after %llu batches", (unsigned long long)b);
  }
  return st;
}

// Every unit must have run: the drains ran outside the batch guard, so check
// each started set's end state on the device (skipped after a failure), join
// its stream to the caller's, then read the checks' results.
template <typename R>
int wf_check_and_join(WfSet<R>* set, const WfConfig& c, const rtwk::TraceArgs<R>& ta, int st) {
  for (uint32_t k = 0; k < c.nsets; ++k) {
    WfSet<R>& S = set[k];
    if (!S.started) continue;
    if (st == RTW_OK) {
      if (rtwk::launch_wf_check_drained(S.seg_a, S.a.seg_resv, c.segs, ta.counter, ta.total_units, S.a.live, S.s) !=
              hipSuccess ||
          hipMemcpyAsync(&c.poll[2 * k], S.a.live, 4, hipMemcpyDeviceToHost, S.s) != hipSuccess || !S.ev[0].e ||
          hipEventRecord(S.ev[0].e, S.s) != hipSuccess)
        st = rtw_fail(RTW_EHIP, "wavefront drain check failed to run");
    }
    if (k > 0 && S.ev[1].e) {  // join: the caller's stream waits for this set
      if (hipEventRecord(S.ev[1].e, S.s) != hipSuccess || hipStreamWaitEvent(c.stream, S.ev[1].e, 0) != hipSuccess) {
        (void)hipStreamSynchronize(S.s);
        if (st == RTW_OK) st = rtw_fail(RTW_EHIP, "wavefront join failed");
      }
    }
  }
  for (uint32_t k = 0; k < c.nsets && st == RTW_OK; ++k) {
    if (hipEventSynchronize(set[k].ev[0].e) != hipSuccess)
      st = rtw_fail(RTW_EHIP, "wavefront drain check failed to run");
    else if (c.poll[2 * k] != 0u)
      st = rtw_fail(RTW_EHIP, "wavefront drain of set %u left %u segments/reservoirs with work undone", k,
                    c.poll[2 * k]);
  }
  return st;
}

}  // namespace

template <typename R>
int rtw_run_wavefront(const rtwk::TraceArgs<R>& ta, const rtw_params* p, unsigned char* ws, const rtwp::WsLayout& L,
                      int dev, size_t lds, hipStream_t stream, bool stats) {
  if (ta.max_depth == 0) {  // rayColor(depth 0) is black (main.zig:105-108): no segment to trace
    if (hipMemsetAsync(ws + L.partial_off, 0, L.partial_bytes, stream) != hipSuccess)
      return rtw_fail(RTW_EHIP, "wavefront: clearing the chunk sums failed");
    return RTW_OK;
  }
  WfConfig c;
  int st = wf_config(c, ta, p, dev, lds, stream, stats);
  if (st != RTW_OK) return st;
  const rtwp::WfSetLayout W = rtwp::wf_set_layout(p);
  WfSet<R> set[kWfMaxSets];
  RtwEvent fork;
  if (!fork.create() || hipEventRecord(fork.e, stream) != hipSuccess)
    st = rtw_fail(RTW_EHIP, "wavefront fork event failed");
  for (uint32_t k = 0; k < c.nsets && st == RTW_OK; ++k) st = wf_set_up(set[k], k, c, ta, ws, L, W, dev, fork.e);
  const auto t_start = Clock::now();
  uint32_t left = st == RTW_OK ? c.nsets : 0u;
  while (left > 0 && st == RTW_OK) {
    // Enqueue one batch on every running set, then look at each set's
    // previous batch (so every stream holds a batch while the host waits).
    for (uint32_t k = 0; k < c.nsets && st == RTW_OK; ++k)
      if (!set[k].done) st = wf_enqueue_batch(set[k], k, c);
    for (uint32_t k = 0; k < c.nsets && st == RTW_OK; ++k)
      if (!set[k].done) st = wf_examine_batch(set[k], k, c, t_start, left);
  }
  return wf_check_and_join(set, c, ta, st);
}
template int rtw_run_wavefront<double>(const rtwk::TraceArgs<double>&, const rtw_params*, unsigned char*,
                                       const rtwp::WsLayout&, int, size_t, hipStream_t, bool);
template int rtw_run_wavefront<float>(const rtwk::TraceArgs<float>&, const rtw_params*, unsigned char*,
                                      const rtwp::WsLayout&, int, size_t, hipStream_t, bool);
