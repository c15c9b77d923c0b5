// rtw_world_build.hpp — the definition of a rebuilt tree (rtw_hip.h
// rtw_world_rebuild), shared by the host build
// (rtw_world_build.cpp) and the rebuild kernels (rtw_world_rebuild.hip) the way
// rtw_world_refit.hpp is shared by the refit: a primitive's Morton key, the
// builder's `need`, the depth cap, the split of a sorted range, the leaf ref,
// a node's place in the refit's schedule and a node's term of the tree cost.
// Host and device; one IEEE operation per operator (-ffp-contract=off); no
// arrays indexed at run time beyond the caller's tables.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rtw_layout.hpp"
#include "rtw_world_refit.hpp"

namespace rtwb {

constexpr uint32_t kFieldBits = 21;              // bits of a key per axis: a 63-bit Morton code
constexpr uint32_t kMaxLevels = rtwk::kBvhStack;  // a rebuilt tree has depth <= cap_of() <= kBvhStack - 1 levels
constexpr uint32_t kTopoBlock = 1024;            // lanes of the single workgroup that splits level by level
// what the host reads back after phase 1: the validation's partial, then depth | nodes per level
constexpr uint32_t kReadbackBytes = rtwr::kPartial * 8 + 4 * (1 + kMaxLevels);

// The builder's `need` loop (rtw_world_pack.cpp Builder::node) at leaves of one:
// median-split levels that `count` primitives still take, ceil(log2 count).
RTWR_HD uint32_t need_of(uint32_t count) {
  uint32_t need = 0;
  for (uint32_t c = count; c > 1u; c = (c + 1u) / 2u) ++need;
  return need;
}
// Depth cap: the per-lane walk's stack when a median tree of the world fits it, else the union walk's.
RTWR_HD uint32_t cap_of(uint32_t n_prims) {
  return need_of(n_prims) <= rtwk::kLaneStack ? rtwk::kLaneStack : rtwk::kBvhStack - 1u;
}

RTWR_HD void centroid(const double lo[3], const double hi[3], double c[3]) {
  c[0] = 0.5 * (lo[0] + hi[0]), c[1] = 0.5 * (lo[1] + hi[1]), c[2] = 0.5 * (lo[2] + hi[2]);
}
// min(2^21 - 1, (uint64)((c - lo) / ext * 2^21)), 0 when ext == 0 (or when the quotient is no number)
RTWR_HD uint64_t key_field(double c, double lo, double ext) {
  if (ext == 0.0) return 0u;
  const double q = (c - lo) / ext * 2097152.0;
  if (!(q >= 0.0)) return 0u;
  if (q >= 2097151.0) return 2097151u;
  return (uint64_t)q;
}
RTWR_HD uint64_t spread3(uint64_t v) {  // bit i of 21 -> bit 3 i
  v &= 0x1FFFFFull;
  v = (v | (v << 32)) & 0x001F00000000FFFFull;
  v = (v | (v << 16)) & 0x001F0000FF0000FFull;
  v = (v | (v << 8)) & 0x100F00F00F00F00Full;
  v = (v | (v << 4)) & 0x10C30C30C30C30C3ull;
  v = (v | (v << 2)) & 0x1249249249249249ull;
  return v;
}
// x's field in bits 2, 5 .. 62, y's in 1, 4 .. 61, z's in 0, 3 .. 60.
// clo / chi: the box of every primitive's centroid.
RTWR_HD uint64_t morton_key(const double c[3], const double clo[3], const double chi[3]) {
  const uint64_t x = key_field(c[0], clo[0], chi[0] - clo[0]);
  const uint64_t y = key_field(c[1], clo[1], chi[1] - clo[1]);
  const uint64_t z = key_field(c[2], clo[2], chi[2] - clo[2]);
  return (spread3(x) << 2) | (spread3(y) << 1) | spread3(z);
}
// The key of list index i from the INPUT numbers (V.a, V.xv), as the boxes are.
RTWR_HD uint64_t key_of(const rtwr::View& V, uint32_t i, const double clo[3], const double chi[3]) {
  double lo[3], hi[3], c[3];
  rtwr::box_of(V, rtwr::prim_meta0(V, V.order[i]), i, lo, hi);
  centroid(lo, hi, c);
  return morton_key(c, clo, chi);
}

RTWR_HD uint32_t highest_bit(uint64_t x) {  // x != 0
  return 63u - (uint32_t)__builtin_clzll(x);
}
// Where the node at depth d that covers [b, e) of the sorted keys (e - b >= 2)
// splits: while a median subtree of the rest still fits the cap, where the
// highest differing key bit changes (the median when every key is equal);
// after that the median.  b < result < e.
RTWR_HD uint32_t split_of(const uint64_t* keys, uint32_t b, uint32_t e, uint32_t d, uint32_t cap) {
  const uint32_t mid = b + (e - b) / 2u;
  if (!(d + need_of(e - b) < cap)) return mid;
  const uint64_t kf = keys[b], kl = keys[e - 1u];
  if (kf == kl) return mid;
  const uint32_t p = highest_bit(kf ^ kl);
  uint32_t lo = b, hi = e - 1u;  // bit p: clear at lo, set at hi; the keys between share every higher bit
  while (hi - lo > 1u) {
    const uint32_t m = lo + (hi - lo) / 2u;
    if ((keys[m] >> p) & 1u) hi = m;
    else lo = m;
  }
  return hi;
}
RTWR_HD uint32_t leaf_ref(uint32_t pos) { return rtwk::kLeafBit | (1u << 23) | pos; }

// The refit's schedule of a rebuilt tree: levels, the deepest first.  Node x of
// level L (records level_off[L] .. level_off[L + 1], breadth-first numbering)
// of a tree of `depth` levels has the label depth - L (the root's is depth, a
// child's is one less than its parent's) and this place in by_height.
RTWR_HD uint32_t sched_label(uint32_t depth, uint32_t level) { return depth - level; }
RTWR_HD uint32_t sched_place(uint32_t n_nodes, uint32_t level_begin, uint32_t level_end, uint32_t x) {
  return (n_nodes - level_end) + (x - level_begin);
}

// Tree cost (rtw_world_bvh_cost): half the surface area of a box, and a node's
// two child boxes as the node table stores them (words 0-11).
RTWR_HD double half_area(double l0, double l1, double l2, double h0, double h1, double h2) {
  const double d0 = h0 - l0, d1 = h1 - l1, d2 = h2 - l2;
  return (d0 * d1 + d1 * d2) + d2 * d0;
}
RTWR_HD double node_cost(const float* nd) {
  return half_area(nd[0], nd[2], nd[4], nd[6], nd[8], nd[10]) + half_area(nd[1], nd[3], nd[5], nd[7], nd[9], nd[11]);
}
RTWR_HD double root_half_area(const float* nd) {
  return half_area(rtwr::fmin32(nd[0], nd[1]), rtwr::fmin32(nd[2], nd[3]), rtwr::fmin32(nd[4], nd[5]),
                   rtwr::fmax32(nd[6], nd[7]), rtwr::fmax32(nd[8], nd[9]), rtwr::fmax32(nd[10], nd[11]));
}

}  // namespace rtwb
