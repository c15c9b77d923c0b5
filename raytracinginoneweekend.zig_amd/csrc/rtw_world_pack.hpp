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
#include "rtw_world_refit.hpp"

namespace rtwp {

struct WorldPack {
  std::vector<unsigned char> blob;  // every table, each at a 256-B aligned offset
  // byte offsets of the tables in the blob (rtwk::WorldView's pointers)
  size_t o_prim = 0, o_xform = 0, o_tex = 0, o_mat = 0, o_perlin = 0, o_image = 0, o_pixels = 0, o_node = 0,
         o_order = 0, o_cull = 0;
  uint32_t n_prims = 0, n_nodes = 0, n_perlins = 0;
  uint32_t view_flags = 0;  // WorldView.flags (kWorldHasSpheres)
  float cull_cmax = 0.0f, cull_rho = 0.0f;  // rtw_cull.hpp Cmax and rho_max over the pretested spheres
  uint32_t feat = 0;        // features used (rtw_world.hip kFeat*): 1 noise, 2 image, 4 transform chains, 8 rects, 64 triangles
  bool has_moving = false;
  double bounds_lo[3] = {0, 0, 0}, bounds_hi[3] = {0, 0, 0};  // box of every primitive (+-inf when empty)
  uint32_t info[4] = {0, 0, 0, 0};  // rtw_world_bvh_info: nodes, leaves, depth, largest leaf
  bool packed = false;  // the BVH carries the refs in its bounds' low bytes too (compact_ref)
  bool has_cull = false;  // a leaf pretest table was built (some leaf ref carries kCullBit)
};

// A child ref (node words 12-13) as the 24 bits the per-lane walk gathers from
// the low bytes of the child's three lower bounds: an interior node index
// < 2^23, or 0x800000 | (count - 1) << 22 | first primitive < 2^22.
uint32_t compact_ref(uint32_t ref);
// pack_refs' rounding of a lower bound, as the packer states it (the refit's
// statement is rtwr::lower_with_low8; tests/native/refit_check.cpp compares them).
float pack_lower_with_low8(float f, uint32_t payload);

// Validates the descriptor (its arrays; `d` itself is not NULL) and builds the
// tables.  flags: RTW_WORLD_LINEAR, RTW_WORLD_DEBUG_BVH (the builder's report
// on stderr).  no_leaf_pretest: leave every leaf without its pretest record (a
// development A/B).  Returns RTW_OK, or the status of the first failed check
// with its message in `msg`.
int pack_world(const rtw_world_desc* d, uint32_t flags, bool no_leaf_pretest, WorldPack& out, std::string& msg);

// ------------------------------------------------------------- refit ----
// What an RTW_WORLD_DYNAMIC world keeps beside its tables, made once from the
// finished WorldPack (rtw_world_refit.cpp; never part of WorldPack::blob):
// the refit's own tables as a second blob, and the host's copy of what an
// update may not change.
struct RefitPack {
  std::vector<unsigned char> blob;  // by_height | heights | plain | cand | mate, each at a 256-B aligned offset
  size_t o_by_height = 0, o_heights = 0, o_plain = 0, o_cand = 0, o_mate = 0;
  // Nodes of height h (1 = both children are leaves ... h_max = the root) are
  // by_height[h_off[h - 1] .. h_off[h]); h_star: the smallest height such that
  // the nodes of height >= h_star number at most 256 (one workgroup).
  std::vector<uint32_t> h_off;
  uint32_t h_max = 0, h_star = 0;
  uint32_t n_xforms = 0;
  std::vector<uint32_t> kind, mat, xf_header;  // per primitive (list order); per transform: n | op << (8 + 4 k)
  std::vector<int32_t> xform;
  std::string msg;  // why the last refit_world refused
};
void make_refit(const rtw_world_desc* d, const WorldPack& k, RefitPack& out);
// The definition of an update's result: the tables, cull_cmax / cull_rho and
// bounds of `k` after the primitives take the numbers a (n_prims x 9, list
// order) and the transforms xv (n_xforms x RTW_MAX_XFORM_OPS x 3, or NULL:
// unchanged).  RTW_EINVAL (k and r untouched, r.msg set) when a used number is
// not finite or a moving sphere has t1 <= t0.
int refit_world(WorldPack& k, RefitPack& r, const double* a, const double* xv);
// The pieces of refit_world that rtw_world_update (rtw_world_capi.hip) shares: the view over
// host blobs, the refusal's message, and the host scalars from the reduced partial.
rtwr::View refit_view(WorldPack& k, RefitPack& r, const double* a, const double* xv);
std::string refit_violation(double bad, double first_bad, uint32_t n_prims);
void refit_scalars(const rtwr::Partial& p, uint32_t n_nodes, float& cull_cmax, float& cull_rho, double lo[3], double hi[3]);
// The host entry's check: kinds, materials, transform indices and op lists equal the world's.
bool same_fixed_fields(const RefitPack& r, const rtw_prim* prims, uint32_t n_prims, const rtw_xform* xforms,
                       uint32_t n_xforms, std::string& msg);


// ----------------------------------------------------------- rebuild ----
// (rtw_world_build.cpp)  The definition of a rebuild's topology:
// from the numbers a / xv, a new stored order (Morton keys, stable from list
// order), a full binary tree over it numbered breadth-first, the order table,
// the records' meta doubles at their new positions, the refs, and the refit's
// tables (candidates judged on the new numbers; the schedule is the tree's
// levels, the deepest first) — everything refit_world(k, r, a, xv) then needs
// to leave the tables of a rebuilt world.  k.info[2] becomes the new depth.
// RTW_UNSUPPORTED unless the tree has leaves of one primitive; RTW_EINVAL as
// refit_world; in both cases k and r are untouched and r.msg is set.
int rebuild_world(WorldPack& k, RefitPack& r, const double* a, const double* xv);
bool rebuild_supported(uint32_t n_prims, uint32_t n_nodes, const uint32_t info[4]);
// h_off / h_max / h_star of r from the nodes per level of a tree of `depth` levels.
void level_schedule(const uint32_t* level_count, uint32_t depth, uint32_t n_nodes, RefitPack& r);

}  // namespace rtwp
