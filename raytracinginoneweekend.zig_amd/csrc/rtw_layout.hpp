// rtw_layout.hpp — constants of the device table layout (rtw_internal.hpp has
// the layout itself), shared by the kernels and the host packers
// (rtw_scene_pack.cpp, rtw_world_pack.cpp).  No HIP: a plain C++ compiler
// builds the packers and their checks (tests/native/).
#pragma once
#include <stdint.h>

namespace rtwk {

// ------------------------------------------------------------ cover scene --
constexpr uint32_t kMoving = 1u;  // meta bit 0
constexpr uint32_t kWide = 2u;    // meta bit 1
constexpr uint32_t kMaxTimeGroups = 64;
constexpr double kWideRadius = 100.0;  // f32 mode: radius >= this -> f64 quadratic

#ifndef RTW_CLUSTER_SLOTS  // (A/B builds override it: 4 or 8)
#define RTW_CLUSTER_SLOTS 8
#endif
constexpr uint32_t kClusterSlots = RTW_CLUSTER_SLOTS;  // slots per cluster (even, divides 64)
static_assert(kClusterSlots % 2 == 0 && 64 % kClusterSlots == 0, "cluster slots");

// ---------------------------------------------------------- general world --
constexpr uint32_t kWorldRec = 16;   // doubles per prim / xform / texture record
constexpr uint32_t kMaxXfOps = 4;    // ops per transform chain (== RTW_MAX_XFORM_OPS)
constexpr uint32_t kNodeWords = 16;  // 32-bit words per BVH node
constexpr uint32_t kLeafBit = 0x80000000u;
constexpr uint32_t kCullBit = 0x40000000u;  // leaf ref: pretest record present
constexpr uint32_t kLeafCountMask = 0x7Fu;  // leaf ref: count = (ref >> 23) & mask
constexpr uint32_t kBvhStack = 32;  // per-wave LDS stack entries (the builder caps the depth)
// per-LANE stack entries of the per-lane traversal (rtw_world.hip closest_lane):
// a BVH of depth <= kLaneStack never overflows it (a push per level at most);
// deeper BVHs take the union walk
constexpr uint32_t kLaneStack = 16;
// The per-lane walk's node cache: the first kNodeCache node records (the top
// of the tree in breadth-first order, rtw_world_pack.cpp top_first) staged in
// LDS once per workgroup; a lane visiting one reads it with ds_read instead of
// three vector loads through the TA/TD pipe that bounds the walk.  0: none —
// the default: 21 records (with RTW_LANE_STACK_LDS 15 to fit four workgroups
// per CU) measured equal on the globe, 31.67 vs 31.29 ms (the walk pays per
// wave iteration, ~41 per segment for ~18 visits per lane, not per lane-load);
// profiles/r06/world_ncache_ab.txt.
#ifndef RTW_NODE_CACHE
#define RTW_NODE_CACHE 0
#endif
constexpr uint32_t kNodeCache = RTW_NODE_CACHE;
#ifndef RTW_MAX_LEAF_PRIMS
#define RTW_MAX_LEAF_PRIMS 2  // BVH leaf size (profiles/r01/world_leaf_ab.txt; experiment builds override it)
#endif
constexpr uint32_t kMaxLeafPrims = RTW_MAX_LEAF_PRIMS;
#ifndef RTW_SAH_BINS
#define RTW_SAH_BINS 256  // bins of the builder's SAH sweep (profiles/r01/world_sah_bins_ab.txt)
#endif
constexpr uint32_t kWorldHasSpheres = 1;  // WorldView.flags
constexpr uint32_t kTailWin = 32;  // world kernel: the last samples of a unit other lanes may trace (ring entries)

// ------------------------------------------- work units and the workspace --
// (what the render plan, rtw_plan.hpp, sizes: the kernels' side is rtw_internal.hpp)
constexpr uint32_t kTileW = 8, kTileH = 8;  // 64 pixels = one wave's batch
constexpr uint32_t kNoiseGrid = 256;  // workgroups of accum_noise_kernel: fixed, so the sum's order never changes
constexpr uint32_t kSegCap = 64;    // wavefront engine: paths per segment (one 64-lane wave round)
constexpr uint32_t kDrainWin = 32;  // wf_drain: samples of a unit dealt ahead of its fold (ring entries per slot)
// A home slot of the wavefront engine, one 32-B record (one memory sector):
// a sample end reads and updates the three fields together (separate arrays
// touched three sectors per access, partially).
struct alignas(32) HomeRec {
  double sum[3];      // f64 chunk sum of the unit's finished samples
  uint32_t unit, s;   // the unit, the sample in flight
};
static_assert(sizeof(HomeRec) == 32, "HomeRec is one 32-B sector");
// One SoA path queue of the wavefront engine: an array per member, in this
// order in the workspace (rtw_plan.cpp wf_set_layout).
template <typename R>
struct PathBuf {
  R *ox, *oy, *oz, *dx, *dy, *dz, *tx, *ty, *tz, *tm;
  uint64_t* rs;
  uint32_t* slot;  // home slot
  uint32_t* dsk;   // depth | (skip + 1) << 16
  int32_t* hk;     // fused engine: the table position of the path's closest hit, -1 = miss; with hk >= 0 the path's
                   // o holds the hit point o + t * d (made where the hit was found: wavefront.hip to_hit_point)
};

}  // namespace rtwk
