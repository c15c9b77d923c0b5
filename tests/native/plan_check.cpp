// The render plan (csrc/rtw_plan.cpp) against the layouts' descriptions:
// every region of a wavefront queue set, of the workspace's counter block and
// of the accumulator's two allocations is 256-B aligned, in order, large
// enough for its elements and ends where the sizes say; the unit arithmetic
// holds; validate_params returns the status of every rejection the library's
// Python tests list (tests/test_capi_cpu.py).  The expected regions are
// restated here from rtw_internal.hpp's WfArgs / PathBuf, not taken from the
// plan.
//
// Grid: engine x precision x wf_sets 0-4 x wf_drain x wf_paths {0, 64, 65,
// 4096, 3 << 18} x image {2x2, 9x9, 96x54, 1200x675, 1200x675 rows 1 + 3k} x
// (spp, chunk) {(1,0), (3,0), (40,7), (500,0), (20,32)}.
//
// usage: plan_check  ->  "plans N checks C violations V", exit 1 if V > 0.
#include <cstdio>
#include <string>
#include <vector>

#include "rtw_layout.hpp"
#include "rtw_plan.hpp"

namespace {

long g_checks = 0, g_viol = 0;
std::string g_plan;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    ++g_checks;                                            \
    if (!(cond) && g_viol++ < 20) {                        \
      fprintf(stderr, "%s: %s: ", g_plan.c_str(), #cond);  \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n");                               \
    }                                                      \
  } while (0)

rtw_params base_params(uint32_t w, uint32_t h, uint32_t spp) {
  rtw_params p{};
  p.width = w, p.height = h, p.spp = spp;
  p.max_depth = 50, p.seed = 42;
  p.row_stride = 1, p.row_count = h;
  p.device = -1;
  return p;
}

struct Want {  // a region as the layout's description has it
  const char* name;
  size_t elems, elem_size;
};

// Alignment, order, capacity and the end of `g` against the regions wanted, in order.
void check_regions(const rtwp::Regions& g, const std::vector<Want>& want, const char* what) {
  CHECK(g.n == want.size(), "%s: %u regions, want %zu", what, g.n, want.size());
  size_t end = 0;  // of the regions so far
  for (uint32_t i = 0; i < g.n && i < want.size(); ++i) {
    const rtwp::Region& r = g.r[i];
    const size_t need = want[i].elems * want[i].elem_size;
    CHECK(r.off % 256 == 0, "%s.%s at %zu", what, want[i].name, r.off);
    CHECK(r.off >= end, "%s.%s at %zu overlaps its predecessor's end %zu", what, want[i].name, r.off, end);
    CHECK(r.elems * r.elem_size >= need, "%s.%s holds %zu B, needs %zu", what, want[i].name, r.elems * r.elem_size, need);
    const size_t next = i + 1 < g.n ? g.r[i + 1].off : g.bytes;
    CHECK(next >= r.off && next - r.off >= need, "%s.%s: %zu B to the next region, needs %zu", what, want[i].name,
          next - r.off, need);
    end = r.off + need;
  }
  if (g.n) {
    const rtwp::Region& l = g.r[g.n - 1];
    CHECK(g.bytes == l.off + ((l.elems * l.elem_size + 255) & ~(size_t)255), "%s ends at %zu", what, g.bytes);
  }
}

void check_wavefront(const rtw_params& p, const rtwp::WsLayout& L) {
  const uint32_t sets = p.wf_sets ? p.wf_sets : RTW_DEFAULT_WF_SETS;
  const uint32_t paths = p.wf_paths ? p.wf_paths : RTW_DEFAULT_WF_PATHS;
  const size_t per_set = (paths + sets - 1) / sets, segs = (per_set + 63) / 64, n = segs * 64;
  const size_t r = p.precision == RTW_PRECISION_F32 ? 4 : 8;
  CHECK(rtwp::wf_sets(&p) == sets && rtwp::wf_segs(&p) == segs, "sets %u segs %u", rtwp::wf_sets(&p), rtwp::wf_segs(&p));
  CHECK(n >= per_set && n < per_set + 64, "%zu slots per set for a share of %zu paths", n, per_set);
  std::vector<Want> want;
  const char* member[14] = {"ox", "oy", "oz", "dx", "dy", "dz", "tx", "ty", "tz", "tm", "rs", "slot", "dsk", "hk"};
  for (int q = 0; q < 2; ++q)
    for (int m = 0; m < 14; ++m) want.push_back({member[m], n, m < 10 ? r : m == 10 ? (size_t)8 : (size_t)4});
  want.push_back({"hit_t", n, r});
  want.push_back({"hit_k", n, 4});
  want.push_back({"home", n, sizeof(rtwk::HomeRec)});
  want.push_back({"seg_a", segs, 4});
  want.push_back({"seg_b", segs, 4});
  want.push_back({"seg_resv", segs, 8});
  const bool ring = p.wf_drain == RTW_WF_DRAIN_SAMPLES;
  if (ring) want.push_back({"drain_buf", n * rtwk::kDrainWin * 3, r});
  const rtwp::WfSetLayout W = rtwp::wf_set_layout(&p);
  check_regions(W.g, want, "set");
  // a queue has one region per PathBuf member; the named regions are where the list has them
  const size_t members = sizeof(rtwk::PathBuf<double>) / sizeof(void*);
  static_assert(sizeof(rtwk::PathBuf<double>) == sizeof(rtwk::PathBuf<float>), "PathBuf: pointers only");
  CHECK(W.queue[0] == 0 && W.queue[1] - W.queue[0] == members && W.hit_t - W.queue[1] == members,
        "queues at %u, %u, hit_t at %u: %zu members", W.queue[0], W.queue[1], W.hit_t, members);
  CHECK(W.hit_k == W.hit_t + 1 && W.home == W.hit_t + 2 && W.seg_a == W.hit_t + 3 && W.seg_b == W.hit_t + 4 &&
            W.seg_resv == W.hit_t + 5, "named regions out of order");
  CHECK(W.drain_buf == (ring ? W.hit_t + 6 : rtwp::WfSetLayout::kNone) && rtwp::wf_per_sample_drain(&p) == ring,
        "drain_buf %u", W.drain_buf);
  CHECK(L.wf_set_bytes == W.g.bytes, "wf_set_bytes %zu, the set ends at %zu", L.wf_set_bytes, W.g.bytes);
  CHECK(L.total == L.wf_off + sets * L.wf_set_bytes, "total %zu", L.total);
}

void check_plan(const rtw_params& p) {
  std::string msg;
  const int st = rtwp::validate_params(&p, msg);
  CHECK(st == RTW_OK, "rejected: %s", msg.c_str());
  if (st != RTW_OK) return;
  // units
  const uint32_t chunk = std::min(p.chunk ? p.chunk : RTW_DEFAULT_CHUNK, p.spp), chunks = (p.spp + chunk - 1) / chunk;
  const uint64_t tiles = (uint64_t)((p.width + 7) / 8) * ((p.row_count + 7) / 8);
  CHECK(rtwp::eff_chunk(&p) == chunk && rtwp::n_chunks(&p) == chunks, "chunk %u x %u", rtwp::eff_chunk(&p), rtwp::n_chunks(&p));
  CHECK((uint64_t)rtwp::tiles_x(&p) * rtwp::tiles_y(&p) == tiles && rtwp::frame_tiles(&p) == tiles, "tiles %u", rtwp::frame_tiles(&p));
  CHECK(rtwp::total_units(&p) == tiles * 64 * chunks && rtwp::total_units(&p) < (1ull << 31), "units %llu",
        (unsigned long long)rtwp::total_units(&p));
  CHECK(rtwp::tile_units(tiles, chunks) == rtwp::total_units(&p), "tile_units");
  // workspace: chunk sums | counter block | queue sets
  const rtwp::WsLayout L = rtwp::ws_layout(&p);
  const size_t npix = (size_t)p.row_count * p.width;
  CHECK(L.partial_off == 0 && L.partial_bytes == chunks * npix * 24, "partial %zu", L.partial_bytes);
  CHECK(L.counter_off % 256 == 0 && L.counter_off >= L.partial_bytes, "counter block at %zu", L.counter_off);
  const size_t cend = L.counter_off + L.counter_bytes;  // what the reset clears
  CHECK(L.live_off >= L.counter_off + 4 && L.live_off + 4 * RTW_MAX_WF_SETS <= L.live_acc_off, "live words at %zu", L.live_off);
  CHECK(L.live_acc_off % 8 == 0 && L.live_acc_off + 8 * RTW_MAX_WF_SETS <= L.stats_off, "live_acc at %zu", L.live_acc_off);
  CHECK(L.stats_off % 8 == 0 && L.stats_off + 32 * 8 <= cend, "stats at %zu, block ends at %zu", L.stats_off, cend);
  CHECK(L.wf_off == cend && L.wf_off % 256 == 0, "queue sets at %zu", L.wf_off);
  CHECK(rtwp::world_ring_off(&p) % 256 == 0 && rtwp::world_ring_off(&p) >= L.total &&
            rtwp::world_ring_off(&p) < L.total + 256, "ring at %zu", rtwp::world_ring_off(&p));
  if (p.engine == RTW_ENGINE_WAVEFRONT)
    check_wavefront(p, L);
  else
    CHECK(L.wf_set_bytes == 0 && L.total == cend, "megakernel total %zu", L.total);
  // the accumulator's allocations
  check_regions(rtwp::accum_layout(&p), {{"sum", npix * 3, 8}, {"stat", npix * 2, 8}, {"noise", 2 * (rtwk::kNoiseGrid + 1), 8}},
                "accum");
  check_regions(rtwp::accum_masked_layout(&p),
                {{"cnt", npix, 4}, {"act", npix, 1}, {"user", npix, 1}, {"tile_mask", (size_t)tiles, 8},
                 {"tile_list", (size_t)tiles, 4}, {"n_active", 2, 4}},
                "masked");
}

void check_rejection(const char* name, const rtw_params& p, int status) {
  g_plan = name;
  std::string msg;
  const int st = rtwp::validate_params(&p, msg);
  CHECK(st == status && !msg.empty(), "status %d (%s), want %d", st, msg.c_str(), status);
}

// The rejections of tests/test_capi_cpu.py (test_render_rejects_bad_params_before_touching_the_gpu,
// test_params_v4_fields_validated), and the unit queue's bound.
void check_rejections() {
  auto with = [](rtw_params p, auto f) {
    f(p);
    return p;
  };
  const rtw_params b = base_params(10, 10, 1);
  check_rejection("width 1", base_params(1, 10, 1), RTW_EINVAL);
  check_rejection("spp 0", base_params(10, 10, 0), RTW_EINVAL);
  check_rejection("row_stride 0", with(b, [](rtw_params& p) { p.row_stride = 0, p.row_count = 1; }), RTW_EINVAL);
  check_rejection("rows past the image", with(b, [](rtw_params& p) { p.row_begin = 9, p.row_stride = 2, p.row_count = 2; }),
                  RTW_EINVAL);
  check_rejection("5000x5000", base_params(5000, 5000, 1), RTW_UNSUPPORTED);
  check_rejection("precision 7", with(b, [](rtw_params& p) { p.precision = 7; }), RTW_EINVAL);
  check_rejection("engine 2", with(b, [](rtw_params& p) { p.engine = 2; }), RTW_EINVAL);
  check_rejection("wf_paths 8", with(b, [](rtw_params& p) { p.engine = RTW_ENGINE_WAVEFRONT, p.wf_paths = 8; }), RTW_EINVAL);
  check_rejection("max_depth 70000", with(b, [](rtw_params& p) { p.engine = RTW_ENGINE_WAVEFRONT, p.max_depth = 70000; }),
                  RTW_UNSUPPORTED);
  g_plan = "params NULL";
  std::string msg;
  CHECK(rtwp::validate_params(nullptr, msg) == RTW_EINVAL && !msg.empty(), "accepted");
  rtw_params v4 = base_params(64, 36, 1);
  v4.engine = RTW_ENGINE_WAVEFRONT;
  struct {
    const char* name;
    uint32_t rtw_params::*field;
    uint32_t value;
  } bad[] = {{"wf_sets 5", &rtw_params::wf_sets, 5},           {"wf_drain 3", &rtw_params::wf_drain, 3},
             {"wf_form 2", &rtw_params::wf_form, 2},           {"world_waves 5", &rtw_params::world_waves, 5},
             {"world_waves 2", &rtw_params::world_waves, 2},   {"world_features 2", &rtw_params::world_features, 2},
             {"world_traversal 3", &rtw_params::world_traversal, 3}, {"wf_bounces 17", &rtw_params::wf_bounces, 17},
             {"wf_passes 65", &rtw_params::wf_passes, 65}};
  for (const auto& x : bad) {
    rtw_params p = v4;
    p.*(x.field) = x.value;
    check_rejection(x.name, p, RTW_EINVAL);
  }
  // 2^24 pixels x 2^20 chunks of one sample: far past the 32-bit unit queue
  check_rejection("units", with(base_params(4096, 4096, 1u << 20), [](rtw_params& p) { p.chunk = 1; }), RTW_UNSUPPORTED);
}

}  // namespace

int main() {
  const uint32_t images[5][4] = {{2, 2, 0, 1}, {9, 9, 0, 1}, {96, 54, 0, 1}, {1200, 675, 0, 1}, {1200, 675, 1, 3}};
  const uint32_t spp_chunk[5][2] = {{1, 0}, {3, 0}, {40, 7}, {500, 0}, {20, 32}};
  const uint32_t wf_paths[5] = {0, 64, 65, 4096, 3u << 18};
  long plans = 0;
  for (uint32_t engine = 0; engine < 2; ++engine)
    for (uint32_t prec = 0; prec < 2; ++prec)
      for (uint32_t sets = 0; sets <= RTW_MAX_WF_SETS; ++sets)
        for (uint32_t drain = 0; drain <= RTW_WF_DRAIN_NONE; ++drain)
          for (uint32_t paths : wf_paths)
            for (const auto& im : images)
              for (const auto& sc : spp_chunk) {
                rtw_params p = base_params(im[0], im[1], sc[0]);
                p.row_begin = im[2], p.row_stride = im[3];
                p.row_count = (im[1] - im[2] + im[3] - 1) / im[3];
                p.chunk = sc[1];
                p.engine = engine, p.precision = prec, p.wf_sets = sets, p.wf_drain = drain, p.wf_paths = paths;
                char name[160];
                snprintf(name, sizeof(name), "engine %u prec %u sets %u drain %u paths %u image %ux%u rows %u+%uk spp %u chunk %u",
                         engine, prec, sets, drain, paths, im[0], im[1], im[2], im[3], sc[0], sc[1]);
                g_plan = name;
                check_plan(p);
                ++plans;
              }
  check_rejections();
  printf("plans %ld checks %ld violations %ld\n", plans, g_checks, g_viol);
  return g_viol ? 1 : 0;
}
