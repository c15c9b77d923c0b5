// rtw_internal.hpp — device-side scene layout and kernel launch interface,
// shared by rtw_trace.hip (kernels) and rtw_capi.hip (C ABI).
//
// HBM layout of a scene (uploaded once by rtw_scene_create):
//   sph_R  : n x 8 R    {c0.x, c0.y, c0.z, dc.x, dc.y, dc.z, r*r, RN(1/r)}   (dc = c1 - c0, in f64)
//   rad_R  : n x R      radius
//   meta   : n x u32    bit0 moving | bit1 wide | bits2-7 time group | bits8-19 material
//                       | bits20-31 original list index (tie-break)
//   perm   : n x u32    original list index -> table position
// Table order: [static wide | static | moving wide | moving] (SceneView g_*
// offsets), each group in list order; sph / meta carry one padding record.
//   mat_R  : nm x 8 R   {albedo.xyz, odd.xyz, fuzz (metal) | RN(1/ir) (dielectric), ir}
//   kind   : nm x u32   rtw_material_kind
//   tg_R   : ng x 4 R   {t0, t1, RN(1/(t1-t0)), 0} per distinct MovingSphere (time0, time1)
//   wide_d : n x 8 f64  f64 copy of sph (f32 mode solves wide spheres in f64)
//   tg_d   : ng x 4 f64
//   cull   : nn_pad/2 x 16 f32  pretest pairs over the narrow spheres in table
//            order (static narrow, then moving narrow; rtw_cull.hpp)
//   cull_tg: nn_pad/2 x u32     time groups of each pair
// R = double (precision 0) and float (precision 1) copies are both kept.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtw_layout.hpp"  // kMoving, kTileW, kSegCap, HomeRec, PathBuf, kNodeWords, ...: the layout's constants (no HIP)

namespace rtwk {

constexpr uint32_t kBatch = 64;             // work units fetched per atomic

template <typename R>
struct SceneView {
  const R* sph;
  const R* rad;
  const uint32_t* meta;
  const R* mat;
  const uint32_t* kind;
  const R* tg;
  const double* wide_d;
  const double* tg_d;
  const uint32_t* perm;
  const float* cull;     // pretest records, nn_pad / 2 pairs x 16 f32 (rtw_trace.hip cull_pair)
  const uint32_t* cull_tg;  // per pair: time group of sphere 2p | (of 2p+1) << 8
  const float* tg_f;     // f32 time groups (t0, t1, 1/(t1-t0), 0) for the pretest
  uint32_t n, nm, ng;
  uint32_t g_static_wide, g_static, g_moving_wide;  // group ends; the moving group ends at n
  uint32_t nn, nn_pad, n_sn;  // narrow spheres (static narrow first), padded to 32; static narrow count
  uint32_t cull_on;           // pretest usable for this scene (rtw_cull.hpp limits)
  float cull_cmax;            // max |c0|_inf + |c1 - c0|_inf over narrow spheres (rounded up)
  float cull_rho;             // max 2 r^2 + 1 over narrow spheres (rounded up)
  // Clustered pretest (f64): the narrow spheres in
  // spatial clusters of <= 8 slots (cluster c = slots 8c..8c+7, padded with
  // dummy slots); a bounding sphere per cluster, pretested first, lets a wave
  // skip every member's pretest when no lane's ray line can meet it.
  const float* ccull;         // pair records in slot order (PairRec, 16 f32 per slot pair); kClusterSlots per cluster
  const uint32_t* ccull_tg;   // per slot pair: time groups (bits 0-15), y-only (16), static pair (17)
  const float* cclus;         // cluster bounding spheres as static pair records (2 clusters per record)
  const uint32_t* cpos;       // slot -> table position (dummy slots: 0)
  const uint32_t* cvalid;     // per 64-slot block: 2 words, bit 31 - r of word h = slot 32h + r real
  uint32_t n_clusters;        // clusters (blocks of 8 -> 64 slots)
  uint32_t cluster_on;        // clusters usable (set per render: camera times within every time group)
  float cull_rho_cl;          // max 2 R^2 + 1 over the cluster bounding spheres (rounded up)
};

template <typename R>
struct TraceArgs {
  SceneView<R> sc;
  R origin[3], horizontal[3], vertical[3], llc[3], cu[3], cv[3];
  R lens_radius, time0, time1;
  R bg[3];
  R tmin;
  R inv_w1, inv_h1;               // RN(1/(W-1)), RN(1/(H-1))
  R pre_k;                        // prefilter bound: tmin / (2.5 * unit roundoff)
  uint32_t W, H, spp, max_depth, chunk, n_chunks;
  uint32_t row_begin, row_stride, row_count, tiles_x;
  uint32_t total_units;
  uint32_t upt_m, upt_sh, tx_m, tx_sh;  // rtwm::udiv magic of units per tile (64 * n_chunks) and tiles_x
  uint32_t unit_order;            // rtw_device.hpp dealt_unit: 0 image order, 1 last-first
  uint32_t primary_on;            // the primary-first loop runs (f64 unmasked; clusters on, one 64-slot block)
  uint32_t tail_on;               // that loop deals a wave's remaining samples to its idle lanes once the queue is
                                  // dry (the launch's LDS then holds trace_tail_lds_bytes more)
  uint32_t empty_on;              // that loop finishes the units of a batch whose tile no camera ray can hit a sphere
                                  // from without tracing them: the slots and the wide spheres fit the 64 lanes of
                                  // the beam pass together, and max_depth >= 1 (a miss adds the background)
  uint32_t claim_waves;           // that loop claims several batches per queue atomic and reuses a tile's beam pass
                                  // (rtw_claim.hpp): kClaimDiv x the waves of the grid; 0: claims of one batch (a
                                  // launch without empty_on, or with a queue too short for a claim of two)
  uint64_t seed_base;            // SplitMix64(seed).next()
  double* partial;                // [n_chunks][row_count*W][3] chunk sums
  uint32_t* counter;              // work-queue head (zeroed before launch)
  unsigned long long* stats;      // counts {samples, segments, skipped} [0..2]; phase cycles [8..13]
  // A masked accumulator pass (rtw_accum.hip): the launch deals only the tiles that hold an
  // active pixel, total_units = active tiles * 64 * n_chunks, and the take maps a dealt tile through
  // tile_list to the frame's tile and skips a unit whose pixel's bit of tile_mask is clear, as it skips
  // the padding units of edge tiles.  Both null in every other render.
  const uint32_t* tile_list;      // [active tiles] frame tile index, ascending
  const uint64_t* tile_mask;      // [frame tiles] bit l: pixel l of the tile (l = 8 * row + column) is active
};

struct FinalizeArgs {
  const double* partial;
  uint8_t* rgb;
  float* mean;
  uint32_t npix, n_chunks;
  double scale;  // 1.0 / spp
};

// Launchers (rtw_trace.hip).  Return hipError_t of the launch.
// mode: 0 = product, 1 = counts (segments/samples), 2 = diagnostic phase stamps
// masked: a masked accumulator pass (TraceArgs::tile_list / tile_mask set; product mode only).
// The kernel has one configuration per (precision, masked): rtw_trace.hip TraceCfg.
hipError_t launch_trace_f64(const TraceArgs<double>& a, uint32_t grid, size_t lds, hipStream_t s, int mode,
                            bool masked);
hipError_t launch_trace_f32(const TraceArgs<float>& a, uint32_t grid, size_t lds, hipStream_t s, int mode,
                            bool masked);
hipError_t launch_finalize(const FinalizeArgs& a, hipStream_t s);
// Resident workgroups per CU for the trace kernel (occupancy query).
int trace_blocks_per_cu(int precision, size_t lds, bool masked);
// Whether that configuration has the primary-first loop (TraceArgs::primary_on may be set for it).
bool trace_primary_first(int precision, bool masked);
// The megakernel's LDS after the scene tables (lds_bytes): per wave, the lanes' home block — unit fields and
// f64 chunk sum, kHomeLdsBytesPerWave — and, with the primary-first loop, the mask of the lane's unit batch:
// which clustered slots its tile's camera rays may hit (two words per lane, bit order of SceneView::cvalid),
// then the wave's current batch's (a copy per lane), kPrimaryLdsBytesPerWave.  (8: alignment of the home block)
constexpr size_t kHomeLdsBytesPerWave = 2560;
// After them the wave's claim words (rtw_claim.hpp): its reserve of claimed batches, the tile of its last
// beam pass with its verdict, that pass's two mask words and its run of proven-empty batches,
// kClaimLdsBytesPerWave.
constexpr size_t kClaimLdsBytesPerWave = 32;
constexpr size_t kPrimaryLdsBytesPerWave = 4 * 64 * 4 + kClaimLdsBytesPerWave;
size_t trace_home_lds_bytes(int precision, bool masked);
constexpr int kTraceBlock = 256;
// The primary-first loop's tail dealing (TraceArgs::tail_on): a block per wave after the workgroup's home
// blocks — per lane the unit's next sample to hand out, the helper's busy word, the dealing list and the
// unit's window of kTailWindow helper lanes (rtw_trace.hip).  0 for a configuration without that loop.
constexpr uint32_t kTailWindow = 4;
constexpr size_t kTailLdsBytesPerWave = (3 + kTailWindow) * 64 * 4;
size_t trace_tail_lds_bytes(int precision, bool masked);

// ---------------------------------------------------------- accumulator --
// rtw_accum.hip: progressive rendering (rtw_hip.h rtw_accum_*).  A pass
// renders its chunk sums into `partial` as a one-shot render does; the fold
// adds them, chunk by chunk in order, to the frame's running f64 sum — the
// additions finalize_kernel performs, in its order — and keeps the per-pixel
// luminance statistic of the full-size chunks for the noise estimate.
struct FoldArgs {
  const double* partial;  // [n_chunks][npix][3] chunk sums of the pass
  double* sum;            // [npix][3] running pixel sum
  double* stat;           // [npix][2] {sum Y, sum Y^2} over the full chunks, Y = luminance of a chunk sum
  uint32_t npix, n_chunks;
  uint32_t n_full;        // the first n_full chunks of the pass hold a full chunk's samples (a short last one: sum only)
};
struct ResolveArgs {
  const double* sum;  // [npix][3]
  uint8_t* rgb;       // [npix][3]
  float* mean;        // [npix][3], optional
  uint32_t npix;
  double scale;       // 1.0 / samples folded
};
struct NoiseArgs {
  const double* stat;  // [npix][2]
  double* part;        // [kNoiseGrid] per-workgroup sums, then [kNoiseGrid] = the frame's noise
  uint32_t npix;
  double m;            // full chunks folded (>= 2)
  double denom;        // m (m - 1) n_c^2
};
// Masked accumulator: per-pixel sample counts and an active set.  act[pix] != 0 while the
// pixel has received every sample so far and has not converged; the tile masks and the ascending list of
// non-empty tiles are derived from it after every change (launch_accum_active).
struct MaskedFoldArgs {
  FoldArgs f;
  const uint8_t* act;  // [npix]
  uint32_t* cnt;       // [npix] samples folded into the pixel
  uint32_t pass_spp;
};
struct ActiveArgs {
  uint8_t* act;            // [npix]
  const uint8_t* user;     // [npix] optional: act &= (user != 0) (rtw_accum_set_mask)
  const double* stat;      // [npix][2]
  const uint32_t* cnt;     // [npix]
  uint64_t* tile_mask;     // [n_tiles]
  uint32_t* tile_list;     // [n_tiles]
  uint32_t* n_active;      // {active tiles, active pixels}
  uint32_t W, rows, tiles_x, n_tiles;
  uint32_t chunk, min_spp;
  double thr;              // tol * tol; <= 0: no criterion
  uint32_t done;           // with from_cnt: act = (cnt == done) first (rtw_accum_load_counts)
  uint32_t from_cnt;
};
struct ResolveCntArgs {
  const double* sum;
  const uint32_t* cnt;
  uint8_t* rgb;
  float* mean;
  uint32_t npix;
};
struct NoiseCntArgs {
  const double* stat;
  const uint32_t* cnt;
  double* part;   // [kNoiseGrid] sums, [kNoiseGrid] = the noise; then [kNoiseGrid] pixel counts, [2 kNoiseGrid + 1] = pixels used
  uint32_t npix, chunk;
};
hipError_t launch_accum_fold(const FoldArgs& a, hipStream_t s);
hipError_t launch_accum_fold_masked(const MaskedFoldArgs& a, hipStream_t s);
hipError_t launch_accum_active(const ActiveArgs& a, hipStream_t s);
hipError_t launch_accum_resolve_cnt(const ResolveCntArgs& a, hipStream_t s);
hipError_t launch_accum_noise_cnt(const NoiseCntArgs& a, hipStream_t s);
hipError_t launch_accum_fill_u32(uint32_t* p, uint32_t n, uint32_t v, hipStream_t s);
hipError_t launch_accum_resolve(const ResolveArgs& a, hipStream_t s);
hipError_t launch_accum_noise(const NoiseArgs& a, hipStream_t s);
// Per-wave LDS slots of coop_reject (rtw_trace.hip CoopSlots: 64 x u64 + 64 x u32).
constexpr size_t kCoopLdsBytes = (kTraceBlock / 64) * 768;

// ------------------------------------------------------ wavefront engine --
// rtw_wavefront.hip (BASELINE.json configs[3]): the same Tier-B render as the
// megakernel, split into per-bounce kernels over SoA path queues in HBM.
// A path = one in-flight sample: its ray, attenuation product, time, RNG
// state, depth and the home slot that owns its (pixel, chunk) unit.  Two
// queues ping-pong: extend(in) writes the closest hit per queue position,
// shade(in -> out) scatters, finishes samples, refills units/samples and
// appends the live paths to `out`.
// The queues are cut into SEGMENTS of kSegCap paths, each owned by one
// persistent wave: a wave always extends / shades its own segments, compacts
// survivors within a segment (no global atomics), deals units from the
// segment's reservoir (one global atomic per kWfBatch units), and a segment
// runs on the same XCD every launch (fixed grid, round-robin dispatch).
// (kSegCap, kDrainWin, HomeRec, PathBuf: rtw_layout.hpp)
template <typename R>
struct WfArgs {
  TraceArgs<R> t;  // MUST stay at offset 0: kargs<R>() reads it
  PathBuf<R> in, out;
  R* hit_t;         // [queue position of `in`] root of the winner
  int32_t* hit_k;   // [queue position of `in`] table position of the winner, -1 = miss
  HomeRec* home;    // [slot] the slot's unit, sample index and f64 chunk sum
  uint32_t* seg_in;    // [segment] live paths in `in`
  uint32_t* seg_out;   // [segment] live paths written to `out` (shade)
  uint32_t* seg_resv;  // [segment][2] unit reservoir [next, end)
  uint32_t* live;      // wf_count: sum of seg_in (host poll word)
  R* drain_buf;        // wf_drain: [slot][kDrainWin][3] radiance of finished samples awaiting their fold (R: the
                       // sample's radiance is an R value; widened to f64 when folded, as the other engines add it)
  uint32_t n_slots, n_segs;
  uint32_t batch;      // units per reservoir refill (one atomic on the device queue)
  uint32_t bounces;    // wf_step: bounce segments per path per launch (>= 1), the path kept in registers between them
  uint32_t passes;     // wf_step: queue passes per launch (>= 1): in -> out, out -> in, ... (every segment through the queues)
  uint32_t* live_acc;  // wf_step (fused): 8-B aligned 64-bit word, (sum of the launch's final segment counts << 20)
                       // + workgroups finished; zero between launches (the last workgroup resets it)
  uint32_t* poll_out;  // wf_step (fused): the host's pinned poll word, written by the launch's last workgroup
  uint32_t hit_form;   // 1: queue `in` holds paths WITH their hit (fused engine: hk, and o = the hit point); the drains
                       // then shade the stored hit first instead of tracing the segment again
};

// The launchers are overloaded on the precision of their WfArgs.
hipError_t launch_wf_generate(const WfArgs<double>& a, uint32_t grid, size_t lds, hipStream_t s);
hipError_t launch_wf_generate(const WfArgs<float>& a, uint32_t grid, size_t lds, hipStream_t s);
hipError_t launch_wf_extend(const WfArgs<double>& a, uint32_t grid, size_t lds, hipStream_t s);
hipError_t launch_wf_extend(const WfArgs<float>& a, uint32_t grid, size_t lds, hipStream_t s);
hipError_t launch_wf_shade(const WfArgs<double>& a, uint32_t grid, size_t lds, hipStream_t s, bool stats);
hipError_t launch_wf_shade(const WfArgs<float>& a, uint32_t grid, size_t lds, hipStream_t s, bool stats);
hipError_t launch_wf_finish(const WfArgs<double>& a, uint32_t grid, size_t lds, hipStream_t s, bool stats);
hipError_t launch_wf_finish(const WfArgs<float>& a, uint32_t grid, size_t lds, hipStream_t s, bool stats);
hipError_t launch_wf_drain(const WfArgs<double>& a, uint32_t grid, size_t lds, hipStream_t s, bool stats);
hipError_t launch_wf_drain(const WfArgs<float>& a, uint32_t grid, size_t lds, hipStream_t s, bool stats);
// Resident workgroups per CU of a bounce kernel (1 = extend, 2 = shade): the
// persistent grid of that kernel is CUs x this.
int wf_blocks_per_cu(int precision, int kernel, size_t lds);
// live = sum of seg_in[0..n_segs) (one workgroup).
hipError_t launch_wf_count(const uint32_t* seg_in, uint32_t n_segs, uint32_t* live, hipStream_t s);
// Fused engine (default): generate + the first closest hit, then one kernel
// per bounce (shade + the next closest hit; the hit travels with the path).
hipError_t launch_wf_generate_hit(const WfArgs<double>& a, uint32_t grid, size_t lds, hipStream_t s);
hipError_t launch_wf_generate_hit(const WfArgs<float>& a, uint32_t grid, size_t lds, hipStream_t s);
hipError_t launch_wf_step(const WfArgs<double>& a, uint32_t grid, size_t lds, hipStream_t s, bool stats);
hipError_t launch_wf_step(const WfArgs<float>& a, uint32_t grid, size_t lds, hipStream_t s, bool stats);
// *bad = violations of the drained state (non-empty segment, unit left in a
// reservoir, queue head below total_units); 0 after a complete frame.
hipError_t launch_wf_check_drained(const uint32_t* seg_in, const uint32_t* resv, uint32_t n_segs, const uint32_t* head,
                                   uint32_t total_units, uint32_t* bad, hipStream_t s);

// ---------------------------------------------------------- world engine --
// rtw_world.hip / rtw_world_capi.hip: the general-world kernel (all scenes
// of main.zig, BASELINE.json configs[4]).  f64 tables in HBM, 16 doubles
// (128 B) per record:
//   prim   : sphere  {c0.xyz, dc.xyz = c1 - c0, r, t0, t1 - t0, r*r, -, -, -, -, meta(2 x u32 x 2)}
//            rect    {a0, a1, b0, b1, k, a1 - a0, b1 - b0, ...,                  meta}
//            meta = {kind | xform+1 << 8, mat, orig list index, -} in doubles 14-15
//   xform  : {u32 n | op_i << (8 + 4 i)}, v[i].xyz at doubles 4 + 3i
//   texture: {u32 kind, perlin, image, -}, color, odd, even, scale at doubles 2, 5, 8, 11
//   material (8 doubles): {u32 kind, tex}, albedo, fuzz, ir at 1, 4, 5
//   perlin : ranvec 256 x 3 f64, then perm 3 x 256 u32 (per perlin)
//   image  : {width, height, byte offset} + one RGBA8 byte pool
//   node   : 64 B, BVH2 with both child boxes in the parent: f32 lo0.xyz, hi0.xyz,
//            lo1.xyz, hi1.xyz (each f64 box bound rounded OUTWARD to f32, so a box only
//            grows), u32 ref0, ref1; ref bit 31 = leaf {first (bits 0-22), count (23-29),
//            bit 30 = the leaf's spheres have a packed-f32 pretest record cull[first]}
//   cull   : 64 B per stored position (used at a leaf's first position): the
//            megakernel's pair record (rtw_device.hpp PairRec) of the leaf's <= 2 spheres
//   order  : list index -> stored position (the NaN fallback's sequential loop)
// Prims are stored in BVH leaf order; `orig` keeps the list index for the
// reference's tie rule (later object wins).
// (record sizes, ref bits, kBvhStack, kLaneStack, kNodeCache, kMaxLeafPrims: rtw_layout.hpp)
// Of the per-lane walk's kLaneStack entries, kLaneStack - 1 are LDS rows: the
// walk keeps the stack's top entry in a register, and a tree of depth D holds at most D pending nodes (one
// sibling per level of the current path: pops take the deepest), so D - 1 rows
// (RTW_LANE_STACK_LDS: the rows built; the default keeps kLaneStack, one to spare)
#ifndef RTW_LANE_STACK_LDS
#define RTW_LANE_STACK_LDS kLaneStack
#endif
constexpr uint32_t kLaneStackLds = RTW_LANE_STACK_LDS;
static_assert(kLaneStackLds + 1 >= kLaneStack, "a depth-kLaneStack tree must fit the LDS rows + the top register");
// per-lane walk: a paused walk keeps its closest hit's stored position + 1 in
// the low kTravPosBits of one LDS word (rtw_world.hip LaneTravRows)
constexpr uint32_t kTravPosBits = 26;

struct WorldView {
  const double* prim;
  const double* xform;
  const double* tex;
  const double* mat;
  const double* perlin;
  const uint32_t* image;   // n_images x {width, height, offset_lo, offset_hi}
  const uint8_t* pixels;
  const float* node;
  const uint32_t* order;
  const float* cull;             // leaf pretest records (kCullBit leaves)
  uint32_t n_prims, n_nodes, n_perlins, flags;
  float cull_cmax, cull_rho;     // rtw_cull.hpp Cmax and rho_max over the pretested spheres
};

struct WorldArgs {
  TraceArgs<double> t;  // MUST stay at offset 0 (kargs<double>()); t.sc unused
  WorldView w;
  double margin;        // BVH test widening (rtw_world_capi.hip bvh_margin)
  unsigned long long* counts;  // stats pass: {samples, segments, node visits, prim tests}
  double* ring;         // tail dealing: [lane of the grid][kTailWin][3] radiance of samples traced for that lane's unit
  uint32_t tail_deal;   // 1: lanes the queue left without a unit trace samples of the wave's other units
  uint32_t lane_yield;  // per-lane traversal: a phase pauses once fewer lanes than this still walk (0: never)
};

// occ: register-allocation target (workgroups per CU): 1 (none), 3 or 4.
// fs: the kernel's feature set, world_feature_set(features of the world, per-lane
// traversal): bits 1 noise texture, 2 image texture, 4 transform chains, 8 rects,
// 16 per-lane BVH traversal (sphere worlds only).
int world_feature_set(uint32_t feat, bool lane, bool packed);
hipError_t launch_world(const WorldArgs& a, uint32_t grid, size_t lds, hipStream_t s, int mode, int occ, int fs);
int world_blocks_per_cu(size_t lds, int occ, int fs);
constexpr int kWorldBlock = 256;
size_t world_lds_bytes(uint32_t n_perlins, int fs);

// ------------------------------------------------------- feature buffers --
// rtw_guides.hip (scenes) / rtw_world.hip (worlds): one rtw_guide per output
// pixel from the pixel's feature ray (rtw_hip.h) — Camera.getRay
// with its random draws replaced by their means, in f64.  One lane per pixel,
// a workgroup = kGuideTileW x kGuideTileH pixels (a wave = one row).
constexpr uint32_t kGuideTileW = 64, kGuideTileH = 4;
struct GuideRay {
  double origin[3], horizontal[3], vertical[3], llc[3];
  double time;   // time0 + 0.5 * (time1 - time0)
  double bg[3];  // a miss's albedo
  uint32_t W, H, row_begin, row_stride, row_count;
  void* out;     // [row_count][W] rtw_guide
};
struct SceneGuideArgs {
  SceneView<double> sc;
  GuideRay r;
};
struct WorldGuideArgs {
  WorldView w;
  GuideRay r;
};
hipError_t launch_scene_guides(const SceneGuideArgs& a, hipStream_t s);
hipError_t launch_world_guides(const WorldGuideArgs& a, bool tri, hipStream_t s);  // tri: the world holds triangles

// ------------------------------------------------------------ ray queries --
// rtw_query.hip (rtw_hip.h "ray queries"): closest hit or
// occlusion of n caller-supplied rays, one ray per lane.  rays: n x rtw_ray
// (9 f64); out: n x rtw_hit (10 x 8 bytes) or n bytes (occlusion).
constexpr int kQueryBlock = 256;
struct WorldQueryArgs {
  WorldView w;
  const double* rays;
  void* out;
  uint32_t n;           // <= 2^31
  uint32_t lane_yield;  // per-lane walk: a phase pauses once fewer lanes than this still walk (while rays remain)
  uint32_t seq_times;   // 1: a BVH over moving spheres (its boxes cover shutter times [0, 1]): a ray of another
                        // time takes the reference's sequential loop
  double reach;         // max |coordinate| of the world's box: the BVH margin of a ray is bvh_margin's with
                        // the ray's own origin (rtw_world_capi.hip)
};
struct SceneQueryArgs {
  SceneView<double> sc;
  const double* rays;
  void* out;
  uint32_t n;
};
// fs: the query kernel's feature set — kFeatAll (15) for the linear loop and the union walk, a per-lane
// sphere set (world_feature_set with lane) for the per-lane walk.
hipError_t launch_world_query(const WorldQueryArgs& a, uint32_t grid, int fs, bool occlusion, hipStream_t s);
hipError_t launch_scene_query(const SceneQueryArgs& a, uint32_t grid, bool occlusion, hipStream_t s);
size_t query_lds_bytes(int fs);
int query_blocks_per_cu(int fs, bool occlusion);

// ---------------------------------------------------------- mirror points --
// rtw_specular.hip (rtw_hip.h "mirror points"): the previous
// point of n hit records, a mirror record's through the walk of its reflected
// ray.  q.rays: the rays the records came from; q.out: n x rtw_hit for the
// reflected rays' records, or null.  fs and the grid: the query kernels' rules.
struct WorldMirrorArgs {
  WorldQueryArgs q;
  const double* hits;     // n x rtw_hit
  const double* a_prev;   // n_prims x 9, list order, or null
  const double* xv_prev;  // n_xforms x kMaxXfOps x 3, or null
  double* prev_p;         // n x 3
  double cam_o[3];        // the previous camera's origin
  uint32_t steps;         // Newton steps (0: the predictor alone)
};
hipError_t launch_world_mirror(const WorldMirrorArgs& a, uint32_t grid, int fs, hipStream_t s);
int mirror_blocks_per_cu(int fs);

}  // namespace rtwk
