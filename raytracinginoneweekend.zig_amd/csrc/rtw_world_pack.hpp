// rtw_world_pack.hpp — the general world's device tables (rtw_internal.hpp
// "world engine" has the layout): validation of an rtw_world_desc, the BVH
// build, the records and the leaf pretest, as one blob that rtw_world_create
// (rtw_world_capi.hip) uploads as it stands.  Host only, no HIP and no
// environment: tests/native/world_pack_check.cpp builds it with a plain C++
// compiler and checks the tables against the descriptor.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "rtw_hip.h"

namespace rtwp {

struct WorldPack {
  std::vector<unsigned char> blob;  // every table, each at a 256-B aligned offset
  // byte offsets of the tables in the blob (rtwk::WorldView's pointers)
  size_t o_prim = 0, o_xform = 0, o_tex = 0, o_mat = 0, o_perlin = 0, o_image = 0, o_pixels = 0, o_node = 0,
         o_order = 0, o_cull = 0;
  uint32_t n_prims = 0, n_nodes = 0, n_perlins = 0;
  uint32_t view_flags = 0;  // WorldView.flags (kWorldHasSpheres)
  float cull_cmax = 0.0f, cull_rho = 0.0f;  // rtw_cull.hpp Cmax and rho_max over the pretested spheres
  uint32_t feat = 0;        // features used (rtw_world.hip kFeat*): 1 noise, 2 image, 4 transform chains, 8 rects
  bool has_moving = false;
  double bounds_lo[3] = {0, 0, 0}, bounds_hi[3] = {0, 0, 0};  // box of every primitive (+-inf when empty)
  uint32_t info[4] = {0, 0, 0, 0};  // rtw_world_bvh_info: nodes, leaves, depth, largest leaf
  bool packed = false;  // the BVH carries the refs in its bounds' low bytes too (compact_ref)
};

// A child ref (node words 12-13) as the 24 bits the per-lane walk gathers from
// the low bytes of the child's three lower bounds: an interior node index
// < 2^23, or 0x800000 | (count - 1) << 22 | first primitive < 2^22.
uint32_t compact_ref(uint32_t ref);

// Validates the descriptor (its arrays; `d` itself is not NULL) and builds the
// tables.  flags: RTW_WORLD_LINEAR, RTW_WORLD_DEBUG_BVH (the builder's report
// on stderr).  no_leaf_pretest: leave every leaf without its pretest record (a
// development A/B).  Returns RTW_OK, or the status of the first failed check
// with its message in `msg`.
int pack_world(const rtw_world_desc* d, uint32_t flags, bool no_leaf_pretest, WorldPack& out, std::string& msg);

}  // namespace rtwp
