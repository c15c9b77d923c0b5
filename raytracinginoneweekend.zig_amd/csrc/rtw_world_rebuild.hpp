// rtw_world_rebuild.hpp — launches of the rebuild kernels (rtw_world_rebuild.hip)
// for rtw_world_rebuild_device and rtw_world_bvh_cost (rtw_world_capi.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "rtw_world_build.hpp"
#include "rtw_world_update.hpp"

namespace rtwk {

// Device pointers of a rebuild.  Everything but `v`'s tables lives in the
// world's rebuild allocation (made at the first rebuild and kept).
struct RebuildArgs {
  rtwr::View v;          // the world's tables and refit tables; a / xv: this call's input
  uint32_t* self;        // n_prims: i -> i (every primitive its own mate in the validation; the sort's values in)
  double* partials;      // n_wg x rtwr::kPartial: the validation's
  double* result;        // the readback (rtwb::kReadbackBytes): the folded partial, then `levels`
  uint32_t* levels;      // depth | nodes per level [rtwb::kMaxLevels]
  double* cpart;         // n_wg x 6: centroid-box partials
  double* cbox;          // 6: the centroid box
  uint64_t* key;         // n_prims: keys by list index
  uint64_t* keys;        // n_prims: sorted
  uint32_t* sorted;      // n_prims: new stored position -> list index
  uint32_t* rng;         // 2 x n_nodes: the sorted range a node covers
  uint32_t* refs;        // 2 x n_nodes: the new child refs
  uint32_t* by_height;   // n_nodes, n_nodes: the new schedule (copied into v's at the commit)
  uint32_t* heights;
  double* meta;          // 3 x n_prims: meta doubles (11, 14, 15) by new position
  void* sort_tmp;        // the radix sort's temporary storage
  size_t sort_bytes;
  uint32_t n_wg;         // ceil(max(n_prims, n_xforms, 1) / 256)
};

hipError_t rebuild_sort_bytes(uint32_t n_prims, size_t* bytes);
// Once, after the allocation: `self`.
hipError_t launch_rebuild_init(const RebuildArgs& a, hipStream_t s);
// Phase 1 after the validation (launch_update_validate on a.partials / a.result
// with v.mate = a.self): centroid box, keys, sort, topology and schedule.
// Writes the rebuild allocation only.
hipError_t launch_rebuild_build(const RebuildArgs& a, hipStream_t s);
// Phase 2 before launch_update_commit: order, meta doubles, refs, candidates,
// mates, the schedule, and zeros in the pretest records of leaves that are no candidates.
hipError_t launch_rebuild_apply(const RebuildArgs& a, hipStream_t s);

// Tree cost: partials (ceil(n_nodes / 256) doubles) and out (1 double) in device memory.
hipError_t launch_bvh_cost(const float* node, uint32_t n_nodes, double* partials, double* out, hipStream_t s);

}  // namespace rtwk
