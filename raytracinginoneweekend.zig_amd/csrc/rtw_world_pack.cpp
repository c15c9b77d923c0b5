// rtw_world_pack.cpp — builds the general world's device tables
// (rtw_world_pack.hpp; layout: rtw_internal.hpp "world engine").  Plain C++:
// no HIP, no environment.
#include "rtw_world_pack.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "rtw_cull.hpp"
#include "rtw_layout.hpp"
#include "rtw_tri.hpp"
#include "rtw_world_box.hpp"
#include "rtw_world_refit.hpp"

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

// struct Box and prim_box (a primitive's world-space bounding box): rtw_world_box.hpp

struct Bvh {
  std::vector<float> nodes;  // kNodeWords per node
  std::vector<uint32_t> order;  // stored position -> original prim index
  uint32_t n_nodes = 0, n_leaves = 0, max_depth = 0, max_leaf = 0;
  bool packed = false;  // pack_refs: the child refs also in the low bits of the lower bounds
};

// The per-lane walk loads a node's 12 bounds (48 B, three 16-B loads) and not
// its refs (words 12-13): each child's ref, as 24 bits (an interior node
// index < 2^23, or 0x800000 | (count - 1) << 22 | first primitive < 2^22),
// rides in the low byte of that child's three lower bounds (words 0 / 2 / 4
// for child 0, 1 / 3 / 5 for child 1; one byte each, gathered by two
// v_perm_b32), each bound moved DOWN to the nearest float whose low byte is
// the payload (< 512 ulps: the box only grows, so the test stays
// conservative; the union walk reads the same bounds and words 12-13).  The per-lane walk's loads are bound by the vector memory pipeline
// (TD busy ~0.85, profiles/r05/world_ta_pmc.txt): one load of four per visit.
float lower_with_low8(float f, uint32_t payload) {  // the largest float <= f whose low byte is `payload`
  uint32_t b;
  std::memcpy(&b, &f, 4);
  if (!(b & 0x80000000u) && b >= 256u && f != 0.0f) {  // positive: smaller bit patterns are smaller
    uint32_t c = (b & ~255u) | payload;
    if (c > b) c -= 256u;
    std::memcpy(&f, &c, 4);
    return f;
  }
  const uint32_t m = b & 0x7FFFFFFFu;  // zero, tiny or negative: a larger magnitude below zero
  uint32_t c = (m & ~255u) | payload;
  if (c < m) c += 256u;
  c |= 0x80000000u;
  std::memcpy(&f, &c, 4);
  return f;
}
// The per-lane walk's node cache (rtw_world.hip, kNodeCache records in LDS)
// holds the first records: renumber so that the top of the tree comes first,
// breadth-first from the root; the other records keep their depth-first order
// (child 0 of an interior node is still its next record below the top).  Only
// the layout changes: every traversal follows refs, so no result can.
void top_first(Bvh& b, uint32_t k) {
  if (b.n_nodes <= 1 || k <= 1) return;
  std::vector<uint32_t> first{0u};
  for (size_t i = 0; i < first.size() && first.size() < k; ++i)
    for (int c = 0; c < 2 && first.size() < k; ++c) {
      uint32_t ref;
      std::memcpy(&ref, b.nodes.data() + (size_t)rtwk::kNodeWords * first[i] + 12 + c, 4);
      if (!(ref & rtwk::kLeafBit)) first.push_back(ref);
    }
  std::vector<uint32_t> id(b.n_nodes, ~0u);
  for (uint32_t i = 0; i < first.size(); ++i) id[first[i]] = i;
  uint32_t next = (uint32_t)first.size();
  for (uint32_t n = 0; n < b.n_nodes; ++n)
    if (id[n] == ~0u) id[n] = next++;
  std::vector<float> out(b.nodes.size(), 0.0f);  // (the same size: the padding record after the last stays)
  for (uint32_t n = 0; n < b.n_nodes; ++n) {
    float* d = out.data() + (size_t)rtwk::kNodeWords * id[n];
    std::memcpy(d, b.nodes.data() + (size_t)rtwk::kNodeWords * n, rtwk::kNodeWords * 4);
    for (int c = 0; c < 2; ++c) {
      uint32_t ref;
      std::memcpy(&ref, d + 12 + c, 4);
      if (!(ref & rtwk::kLeafBit)) {
        ref = id[ref];
        std::memcpy(d + 12 + c, &ref, 4);
      }
    }
  }
  b.nodes.swap(out);
}

bool pack_refs(Bvh& b, uint32_t n_prims, bool debug) {
  if (b.n_nodes >= 0x800000u || n_prims >= 0x400000u || b.max_leaf > 2u) return false;
  std::vector<float> packed(b.nodes);
  for (uint32_t n = 0; n < b.n_nodes; ++n) {
    float* nd = packed.data() + (size_t)rtwk::kNodeWords * n;
    for (int c = 0; c < 2; ++c) {
      uint32_t r;
      std::memcpy(&r, nd + 12 + c, 4);
      const uint32_t v = compact_ref(r);
      for (int k = 0; k < 3; ++k) {
        const float old = nd[2 * k + c], nw = lower_with_low8(old, (v >> (8 * k)) & 255u);
        if (!(nw <= old) || !std::isfinite(nw)) return false;  // (never: the bounds are finite)
        nd[2 * k + c] = nw;
      }
    }
  }
  if (debug) {  // the device's gather (rtw_world.hip trace_phase PACKED) restated, against every ref
    uint32_t bad = 0, worst = 0;
    for (uint32_t n = 0; n < b.n_nodes; ++n) {
      const float* nd = packed.data() + (size_t)rtwk::kNodeWords * n;
      const float* od = b.nodes.data() + (size_t)rtwk::kNodeWords * n;
      for (int c = 0; c < 2; ++c) {
        uint32_t r, w[3], v = 0;
        std::memcpy(&r, nd + 12 + c, 4);
        for (int k = 0; k < 3; ++k) {
          std::memcpy(&w[k], nd + 2 * k + c, 4);
          v |= (w[k] & 255u) << (8 * k);
          uint32_t ob;
          std::memcpy(&ob, od + 2 * k + c, 4);
          const bool neg = (w[k] | ob) & 0x80000000u;  // ulps between the two (same-sign or across zero)
          const uint32_t d = neg ? (w[k] & 0x7FFFFFFFu) + ((ob & 0x80000000u) ? 0u - (ob & 0x7FFFFFFFu) : ob)
                                 : ob - w[k];
          worst = std::max(worst, d);
          if (!(nd[2 * k + c] <= od[2 * k + c])) ++bad;
        }
        if (v != compact_ref(r)) ++bad;
      }
    }
    fprintf(stderr, "[rtw bvh] packed refs: %u nodes, %u mismatches, bounds moved down by <= %u ulps\n", b.n_nodes,
            bad, worst);
  }
  b.nodes.swap(packed);
  b.packed = true;
  return true;
}

// Leaf size: worlds of >= kLeafOneMin primitives (those AUTO walks per lane:
// >= 2 x kLaneNodes) get leaves of ONE primitive, smaller ones kMaxLeafPrims.
// Per lane, a leaf's primitives are tested one after another by the lanes
// that reach it: the globe at leaf 1 vs 2 is +4.3 % (1.98 vs 3.45 primitive
// tests, 17.6 vs 16.3 node visits per segment), 10 of 10 alternations; leaves
// of 3 and 4 are slower; the union walk on scene 1 (48 primitives) prefers 2
// (-6 % at 1): profiles/r05/world_leaf_ab.txt.
constexpr size_t kLeafOneMin = 512;

class Builder {
 public:
  // depth_cap: the tree's depth (interior levels on a root-to-leaf path) stays
  // <= depth_cap - 1 for the union walk's kBvhStack and <= depth_cap for
  // depth_cap = kLaneStack (the per-lane walk's rebuild, below): SAH splits
  // while a median subtree of the rest still fits, median splits after that.
  Builder(const std::vector<Box>& boxes, Bvh& out, uint32_t depth_cap = rtwk::kBvhStack)
      : boxes_(boxes), out_(out), leaf_max_(boxes.size() >= kLeafOneMin ? 1u : rtwk::kMaxLeafPrims),
        cap_(depth_cap), lane_cap_(depth_cap != rtwk::kBvhStack) {
    idx_.resize(boxes.size());
    for (size_t i = 0; i < idx_.size(); ++i) idx_[i] = (uint32_t)i;
    for (const Box& b : boxes) {
      double m[3];
      for (int k = 0; k < 3; ++k) m[k] = 0.5 * (b.lo[k] + b.hi[k]);
      cent_.push_back({m[0], m[1], m[2]});
    }
  }
  void run() {
    const uint32_t root = alloc();
    node(root, 0, (uint32_t)idx_.size(), 0);
    out_.order = idx_;
  }

 private:
  const std::vector<Box>& boxes_;
  Bvh& out_;
  const uint32_t leaf_max_;  // primitives per leaf (<= rtwk::kMaxLeafPrims)
  const uint32_t cap_;       // depth cap (see the constructor)
  const bool lane_cap_;      // the per-lane walk's cap: SAH while depth + need < cap (else + 2 < cap)
  std::vector<uint32_t> idx_;
  std::vector<std::array<double, 3>> cent_;

  uint32_t alloc() {
    out_.nodes.resize(out_.nodes.size() + rtwk::kNodeWords, 0.0f);
    return out_.n_nodes++;
  }
  Box range_box(uint32_t b, uint32_t e) const {
    Box r;
    for (uint32_t i = b; i < e; ++i) r.grow(boxes_[idx_[i]]);
    return r;
  }
  uint32_t leaf(uint32_t b, uint32_t e) {
    out_.n_leaves++;
    out_.max_leaf = std::max(out_.max_leaf, e - b);
    return rtwk::kLeafBit | ((e - b) << 23) | b;
  }
  // Binned SAH split of [b, e); falls back to the median of the widest axis.
  uint32_t split(uint32_t b, uint32_t e, bool sah) {
    Box cb;
    for (uint32_t i = b; i < e; ++i) cb.grow(cent_[idx_[i]].data());
    int axis = 0;
    for (int k = 1; k < 3; ++k)
      if (cb.hi[k] - cb.lo[k] > cb.hi[axis] - cb.lo[axis]) axis = k;
    if (sah && cb.hi[axis] > cb.lo[axis]) {
      constexpr int kBins = RTW_SAH_BINS;  // (rtw_layout.hpp)
      double best = INFINITY;
      int best_axis = -1, best_bin = -1;
      for (int k = 0; k < 3; ++k) {
        const double ext = cb.hi[k] - cb.lo[k];
        if (!(ext > 0)) continue;
        Box bb[kBins];
        uint32_t cnt[kBins] = {0};
        for (uint32_t i = b; i < e; ++i) {
          int t = (int)((cent_[idx_[i]][k] - cb.lo[k]) / ext * kBins);
          t = std::min(std::max(t, 0), kBins - 1);
          bb[t].grow(boxes_[idx_[i]]);
          cnt[t]++;
        }
        Box left[kBins];
        uint32_t lc[kBins];
        Box acc;
        uint32_t ac = 0;
        for (int t = 0; t < kBins; ++t) acc.grow(bb[t]), ac += cnt[t], left[t] = acc, lc[t] = ac;
        acc = Box();
        ac = 0;
        for (int t = kBins - 1; t > 0; --t) {
          acc.grow(bb[t]);
          ac += cnt[t];
          const double cost = left[t - 1].area() * lc[t - 1] + acc.area() * ac;
          if (lc[t - 1] > 0 && ac > 0 && cost < best) best = cost, best_axis = k, best_bin = t;
        }
      }
      if (best_axis >= 0) {
        const double ext = cb.hi[best_axis] - cb.lo[best_axis];
        auto mid = std::partition(idx_.begin() + b, idx_.begin() + e, [&](uint32_t i) {
          int t = (int)((cent_[i][best_axis] - cb.lo[best_axis]) / ext * kBins);
          return std::min(std::max(t, 0), kBins - 1) < best_bin;
        });
        const uint32_t m = (uint32_t)(mid - idx_.begin());
        if (m > b && m < e) return m;
      }
    }
    const uint32_t m = b + (e - b) / 2;
    std::nth_element(idx_.begin() + b, idx_.begin() + m, idx_.begin() + e,
                     [&](uint32_t x, uint32_t y) { return cent_[x][axis] < cent_[y][axis]; });
    return m;
  }
  uint32_t child(uint32_t b, uint32_t e, uint32_t depth) {
    // Leaves: few primitives, or the depth cap of the per-lane LDS stack
    // (node() switches to median splits while they still fit the cap).
    if (e - b <= leaf_max_ || (depth >= (lane_cap_ ? cap_ : cap_ - 1) && e - b <= rtwk::kLeafCountMask))
      return leaf(b, e);
    const uint32_t n = alloc();
    node(n, b, e, depth);
    return n;
  }
  void node(uint32_t n, uint32_t b, uint32_t e, uint32_t depth) {
    out_.max_depth = std::max(out_.max_depth, depth + 1);
    uint32_t m;
    if (e - b <= leaf_max_) {  // root of a tiny world: one leaf + an empty one
      m = e;
    } else {
      // SAH while the median-split depth of the rest still fits the stack.
      uint32_t need = 0;
      for (uint32_t c = e - b; c > leaf_max_; c = (c + 1) / 2) ++need;
      m = split(b, e, lane_cap_ ? depth + need < cap_ : depth + need + 2 < cap_);
    }
    // Child 0 is built first, so an interior child 0 is record n + 1, the line
    // the traversal loads with node n (rtw_world.hip RTW_WORLD_TOUCH_NEXT).
    // (The child of larger surface area first instead: equal, profiles/r04/
    // world_touch_next_ab.txt.)
    const uint32_t lo0 = b, hi0 = m, lo1 = m, hi1 = e;
    const uint32_t c0 = m == e ? leaf(b, e) : child(lo0, hi0, depth + 1);
    const uint32_t c1 = m == e ? (rtwk::kLeafBit | e) : child(lo1, hi1, depth + 1);
    const Box b0 = range_box(lo0, hi0), b1 = range_box(lo1, hi1);
    float* nd = out_.nodes.data() + (size_t)rtwk::kNodeWords * n;
    using rtwr::down;  // largest float <= x
    using rtwr::up;    // smallest float >= x
    for (int k = 0; k < 3; ++k) {  // {lo0, lo1} and {hi0, hi1} pairs per axis (packed-f32 operands)
      nd[2 * k] = down(b0.lo[k]), nd[2 * k + 1] = down(b1.lo[k]);
      nd[6 + 2 * k] = up(b0.hi[k]), nd[7 + 2 * k] = up(b1.hi[k]);
    }
    uint32_t refs[2] = {c0, c1};
    std::memcpy(nd + 12, refs, sizeof(refs));
  }
};

}  // namespace

uint32_t compact_ref(uint32_t r) { return rtwr::compact_ref(r); }
float pack_lower_with_low8(float f, uint32_t payload) { return lower_with_low8(f, payload); }

int pack_world(const rtw_world_desc* d, uint32_t flags, bool no_leaf_pretest, WorldPack& out, std::string& msg) {
  if ((d->n_prims && !d->prims) || (d->n_xforms && !d->xforms) || (d->n_textures && !d->textures) ||
      (d->n_mats && !d->mats) || (d->n_perlins && !d->perlins) || (d->n_images && !d->images))
    return fail(msg, RTW_EINVAL, "rtw_world_create: NULL array with a non-zero count");
  if (d->n_prims >= (1u << 23)) return fail(msg, RTW_UNSUPPORTED, "%u primitives exceed 2^23", d->n_prims);
  for (uint32_t i = 0; i < d->n_xforms; ++i) {
    if (d->xforms[i].n > RTW_MAX_XFORM_OPS) return fail(msg, RTW_EINVAL, "xform %u: %u ops", i, d->xforms[i].n);
    for (uint32_t k = 0; k < d->xforms[i].n; ++k)
      if (d->xforms[i].op[k] > RTW_XF_ROTATE_Y) return fail(msg, RTW_EINVAL, "xform %u: op %u", i, d->xforms[i].op[k]);
  }
  for (uint32_t i = 0; i < d->n_images; ++i)
    if (!d->images[i].rgba || !d->images[i].width || !d->images[i].height)
      return fail(msg, RTW_EINVAL, "image %u is empty", i);
  for (uint32_t i = 0; i < d->n_textures; ++i) {
    const rtw_texture& t = d->textures[i];
    if (t.kind > RTW_TEX_IMAGE) return fail(msg, RTW_EINVAL, "texture %u: kind %u", i, t.kind);
    if (t.kind == RTW_TEX_NOISE && t.perlin >= d->n_perlins) return fail(msg, RTW_EINVAL, "texture %u: perlin", i);
    if (t.kind == RTW_TEX_IMAGE && t.image >= d->n_images) return fail(msg, RTW_EINVAL, "texture %u: image", i);
  }
  for (uint32_t i = 0; i < d->n_mats; ++i) {
    const rtw_wmaterial& m = d->mats[i];
    if (m.kind > RTW_WMAT_LIGHT) return fail(msg, RTW_EINVAL, "material %u: kind %u", i, m.kind);
    if ((m.kind == RTW_WMAT_LAMBERT || m.kind == RTW_WMAT_LIGHT) && m.tex >= d->n_textures)
      return fail(msg, RTW_EINVAL, "material %u: texture %u >= %u", i, m.tex, d->n_textures);
  }
  WorldPack wp;
  Box bounds;
  std::vector<Box> boxes(d->n_prims);
  for (uint32_t i = 0; i < d->n_prims; ++i) {
    const rtw_prim& p = d->prims[i];
    if (p.kind > RTW_PRIM_TRIANGLE || p.mat >= d->n_mats || p.xform >= (int32_t)d->n_xforms || p.xform < -1) {
      return fail(msg, RTW_EINVAL, "prim %u: kind %u / material %u / xform %d out of range", i, p.kind, p.mat, p.xform);
    }
    // MovingSphere.center divides by time1 - time0 (hittable.zig:219-221): an
    // empty or reversed shutter gives a NaN centre, whose box no BVH node
    // could hold (the BVH would prune what the linear list tests).
    if (p.kind == RTW_PRIM_MOVING_SPHERE && !(p.a[8] > p.a[7])) {
      return fail(msg, RTW_EINVAL, "prim %u: moving sphere needs time1 > time0 (got %g, %g)", i, p.a[7], p.a[8]);
    }
    // A triangle needs finite vertices and a non-zero, finite area (rtw_tri.hpp derive): its
    // normal divides by the area.
    if (p.kind == RTW_PRIM_TRIANGLE) {
      double nn[3], hh;
      bool fin = true;
      for (int k = 0; k < 9; ++k) fin = fin && rtwr::finite(p.a[k]);
      if (!fin || !rtwtri::derive(p.a, nn, hh))
        return fail(msg, RTW_EINVAL, "prim %u: triangle with a non-finite vertex or zero area", i);
      wp.feat |= 64u;
    }
    boxes[i] = prim_box(p, p.xform >= 0 ? &d->xforms[p.xform] : nullptr);
    bounds.grow(boxes[i]);
    wp.has_moving |= p.kind == RTW_PRIM_MOVING_SPHERE;
    if (p.xform >= 0) wp.feat |= 4u;
    if (p.kind >= RTW_PRIM_XY_RECT && p.kind <= RTW_PRIM_YZ_RECT) wp.feat |= 8u;
  }
  Bvh bvh;
  // Small worlds (<= kLinearMax primitives: the Cornell box, the Perlin and
  // earth scenes) run the wave-uniform linear loop: every lane tests the same
  // scalar-loaded record, which beat the divergent per-lane BVH walk on
  // MI355X; RTW_WORLD_LINEAR forces it for any size.
  constexpr uint32_t kLinearMax = 32;
  const bool use_bvh = !(flags & RTW_WORLD_LINEAR) && d->n_prims > kLinearMax;
  if (use_bvh) {
    Builder(boxes, bvh).run();
    // The per-lane walk (sphere worlds of >= kLeafOneMin primitives, leaves
    // of one) keeps its stack in kLaneStack LDS entries per lane: a tree
    // deeper than that is rebuilt with SAH splits only while a median subtree
    // of the rest still fits (depth <= kLaneStack), so the lane walk stays
    // available; the globe's SAH tree (depth 16) is already within it.
    const uint32_t unconstrained_depth = bvh.max_depth;
    if (bvh.max_leaf == 1 && bvh.max_depth > rtwk::kLaneStack) {
      Bvh capped;
      Builder(boxes, capped, rtwk::kLaneStack).run();
      if (capped.max_depth <= rtwk::kLaneStack && capped.max_leaf == 1) bvh = std::move(capped);
    }
    if (flags & RTW_WORLD_DEBUG_BVH)
      fprintf(stderr, "[rtw bvh] %u nodes, depth %u (unconstrained SAH: %u), max leaf %u\n", bvh.n_nodes,
              bvh.max_depth, unconstrained_depth, bvh.max_leaf);
    if (flags & RTW_WORLD_DEBUG_BVH) {  // root's two children: leaf (prims) or node, and their boxes
      for (int c = 0; c < 2; ++c) {
        uint32_t ref;
        std::memcpy(&ref, bvh.nodes.data() + 12 + c, 4);
        const float* nd = bvh.nodes.data();
        fprintf(stderr, "[rtw bvh] root child %d: %s %u, box x [%g, %g] y [%g, %g] z [%g, %g]\n", c,
                (ref & rtwk::kLeafBit) ? "leaf of" : "node", (ref & rtwk::kLeafBit) ? (ref >> 23) & rtwk::kLeafCountMask : ref,
                nd[0 + c], nd[6 + c], nd[2 + c], nd[8 + c], nd[4 + c], nd[10 + c]);
      }
    }
    // (leaf-of-one trees are the per-lane walk's: its node cache wants the top first)
    if (bvh.max_leaf == 1) top_first(bvh, rtwk::kNodeCache);
    (void)pack_refs(bvh, d->n_prims, (flags & RTW_WORLD_DEBUG_BVH) != 0);  // (after the diagnostic: it prints the boxes as built)
  } else {
    for (uint32_t i = 0; i < d->n_prims; ++i) bvh.order.push_back(i);
  }
  // Device records, in stored (leaf) order; `order_dev` maps list index -> stored position.
  const uint32_t n = d->n_prims;
  std::vector<double> prim((size_t)rtwk::kWorldRec * (n + 1), 0.0);  // + a zero padding record (prefetch)
  std::vector<uint32_t> list_to_pos(n);
  for (uint32_t pos = 0; pos < n; ++pos) {
    const uint32_t li = bvh.order[pos];
    list_to_pos[li] = pos;
    const rtw_prim& p = d->prims[li];
    double* r = prim.data() + (size_t)rtwk::kWorldRec * pos;
    if (p.kind == RTW_PRIM_TRIANGLE)
      (void)rtwr::fill_record_tri(p.a, r);  // doubles 0-10, 12, 13
    else
      rtwr::fill_record(p.kind, p.a, r);  // doubles 0-10 (shared with the refit)
    const uint32_t meta[4] = {p.kind | ((uint32_t)(p.xform + 1) << 8), p.mat, li, 0u};
    std::memcpy(r + 14, meta, sizeof(meta));
    // the kind and list index again in double 11, so the per-lane walk's root
    // test reads doubles 0-11 only: six 16-B loads per primitive, not seven
    // (rtw_world.hip load_rec_lane)
    const uint32_t meta_lane[2] = {meta[0], meta[2]};
    std::memcpy(r + 11, meta_lane, sizeof(meta_lane));
  }
  // Leaf pretest records (rtw_cull.hpp, the megakernel's packed-f32 bound):
  // a BVH leaf of <= 2 spheres that are untransformed, narrow (|r| < 100) and
  // static or moving over the shutter [0, 1] (their f32 time fraction is the
  // ray's f32 time, as in the cover scene) gets the pair record of its
  // spheres at cull[first] and kCullBit in its ref; the kernel skips a
  // sphere's exact test when no lane's pretest survives.
  std::vector<float> cull;
  float cull_cmax = 0.0f, cull_rho = 0.0f;
  if (use_bvh) {
    auto eligible = [&](uint32_t pos) {
      const rtw_prim& p = d->prims[bvh.order[pos]];
      return rtwr::eligible(p.kind | ((uint32_t)(p.xform + 1) << 8), p.a);
    };
    std::vector<uint32_t> leaf_refs;  // (node, child) slots whose leaf qualifies
    double cmax_c = 0.0, cmax_d = 0.0, rho_max = 1.0;
    for (uint32_t nd = 0; nd < bvh.n_nodes; ++nd) {
      for (uint32_t c = 0; c < 2; ++c) {
        uint32_t ref;
        std::memcpy(&ref, bvh.nodes.data() + (size_t)rtwk::kNodeWords * nd + 12 + c, 4);
        const uint32_t first = ref & 0x7FFFFFu, cnt = (ref >> 23) & rtwk::kLeafCountMask;
        if (!(ref & rtwk::kLeafBit) || cnt == 0 || cnt > 2) continue;
        bool ok = true;
        for (uint32_t k = first; k < first + cnt; ++k) ok = ok && eligible(k);
        if (!ok) continue;
        leaf_refs.push_back(2 * nd + c);
        for (uint32_t k = first; k < first + cnt; ++k) {
          const double* r = prim.data() + (size_t)rtwk::kWorldRec * k;
          for (int j = 0; j < 3; ++j) cmax_c = std::max(cmax_c, std::fabs(r[j])), cmax_d = std::max(cmax_d, std::fabs(r[3 + j]));
          rho_max = std::max(rho_max, 2.0 * r[9] + 1.0);
        }
      }
    }
    cull_cmax = std::nextafter((float)(cmax_c + cmax_d), INFINITY);
    cull_rho = std::nextafter((float)rho_max, INFINITY);
    if (!leaf_refs.empty() && cull_cmax <= rtwc::kCmaxLimit && !no_leaf_pretest) {
      cull.assign((size_t)16 * n, 0.0f);
      for (uint32_t slot : leaf_refs) {
        float* nw = bvh.nodes.data() + (size_t)rtwk::kNodeWords * (slot / 2) + 12 + (slot & 1);
        uint32_t ref;
        std::memcpy(&ref, nw, 4);
        const uint32_t first = ref & 0x7FFFFFu, cnt = (ref >> 23) & rtwk::kLeafCountMask;
        for (uint32_t j = 0; j < cnt; ++j) {  // sphere j of the leaf -> lane j of each f2
          rtwr::fill_cull(cull.data() + (size_t)16 * first, j, prim.data() + (size_t)rtwk::kWorldRec * (first + j));
        }
        ref |= rtwk::kCullBit;  // (cnt <= 2 here, so no ref is all ones: the traversal's kNoRef, rtw_world.hip)
        std::memcpy(nw, &ref, 4);
      }
    }
  }
  std::vector<double> xf((size_t)rtwk::kWorldRec * std::max(d->n_xforms, 1u), 0.0);
  for (uint32_t i = 0; i < d->n_xforms; ++i) {
    double* r = xf.data() + (size_t)rtwk::kWorldRec * i;
    uint32_t h = d->xforms[i].n;
    for (uint32_t k = 0; k < d->xforms[i].n; ++k) {
      h |= d->xforms[i].op[k] << (8 + 4 * k);
      for (int c = 0; c < 3; ++c) r[4 + 3 * k + c] = d->xforms[i].v[k][c];
    }
    std::memcpy(r, &h, 4);
  }
  std::vector<double> tex((size_t)rtwk::kWorldRec * std::max(d->n_textures, 1u), 0.0);
  for (uint32_t i = 0; i < d->n_textures; ++i) {
    const rtw_texture& t = d->textures[i];
    double* r = tex.data() + (size_t)rtwk::kWorldRec * i;
    const uint32_t h[4] = {t.kind, t.perlin, t.image, 0u};
    std::memcpy(r, h, sizeof(h));
    for (int c = 0; c < 3; ++c) r[2 + c] = t.color[c], r[5 + c] = t.odd[c], r[8 + c] = t.even[c];
    r[11] = t.scale;
  }
  std::vector<double> mat((size_t)8 * std::max(d->n_mats, 1u), 0.0);
  for (uint32_t i = 0; i < d->n_mats; ++i) {
    const rtw_wmaterial& m = d->mats[i];
    double* r = mat.data() + (size_t)8 * i;
    const uint32_t h[2] = {m.kind, m.tex};
    std::memcpy(r, h, sizeof(h));
    for (int c = 0; c < 3; ++c) r[1 + c] = m.albedo[c];
    r[4] = m.fuzz, r[5] = m.ir;
  }
  constexpr size_t kPerlinDoubles = 256 * 3 + 384;
  std::vector<double> perl(kPerlinDoubles * std::max(d->n_perlins, 1u), 0.0);
  for (uint32_t i = 0; i < d->n_perlins; ++i) {
    double* r = perl.data() + kPerlinDoubles * i;
    for (int j = 0; j < 256; ++j)
      for (int c = 0; c < 3; ++c) r[3 * j + c] = d->perlins[i].ranvec[j][c];
    std::memcpy(r + 256 * 3, d->perlins[i].perm, sizeof(d->perlins[i].perm));
  }
  std::vector<uint32_t> img(4 * std::max(d->n_images, 1u), 0u);
  size_t pix_bytes = 0;
  for (uint32_t i = 0; i < d->n_images; ++i) {
    img[4 * i] = d->images[i].width, img[4 * i + 1] = d->images[i].height;
    img[4 * i + 2] = (uint32_t)pix_bytes, img[4 * i + 3] = (uint32_t)(pix_bytes >> 32);
    pix_bytes += (size_t)d->images[i].width * d->images[i].height * 4;
  }
  // One blob: prim | xform | tex | mat | perlin | image | pixels | nodes | order | cull,
  // each at a 256-B aligned offset; `room`: a table's size where it is more than its data.
  auto put = [&](size_t& o, const auto& v, size_t room = 0) {
    const size_t bytes = v.size() * sizeof(v[0]);
    o = wp.blob.size();
    wp.blob.resize(o + ((std::max(bytes, room) + 255) & ~(size_t)255), 0);
    if (bytes) std::memcpy(wp.blob.data() + o, v.data(), bytes);
  };
  put(wp.o_prim, prim), put(wp.o_xform, xf), put(wp.o_tex, tex), put(wp.o_mat, mat), put(wp.o_perlin, perl);
  put(wp.o_image, img);
  put(wp.o_pixels, std::vector<unsigned char>(), std::max(pix_bytes, (size_t)4));
  for (uint32_t i = 0; i < d->n_images; ++i)
    std::memcpy(wp.blob.data() + wp.o_pixels + ((size_t)img[4 * i + 2] | ((size_t)img[4 * i + 3] << 32)),
                d->images[i].rgba, (size_t)d->images[i].width * d->images[i].height * 4);
  // (+ two zero padding records: the traversal may load the records after the last)
  put(wp.o_node, bvh.nodes, bvh.nodes.size() * 4 + 2 * (size_t)rtwk::kNodeWords * 4);
  put(wp.o_order, list_to_pos, 4);
  put(wp.o_cull, cull, 4);
  wp.n_prims = n, wp.n_nodes = bvh.n_nodes, wp.n_perlins = d->n_perlins;
  for (uint32_t i = 0; i < n; ++i)
    if (d->prims[i].kind <= RTW_PRIM_MOVING_SPHERE) wp.view_flags |= rtwk::kWorldHasSpheres;
  wp.cull_cmax = cull_cmax, wp.cull_rho = cull_rho;
  for (uint32_t i = 0; i < d->n_textures; ++i)
    wp.feat |= d->textures[i].kind == RTW_TEX_NOISE ? 1u : (d->textures[i].kind == RTW_TEX_IMAGE ? 2u : 0u);
  for (int c = 0; c < 3; ++c) wp.bounds_lo[c] = bounds.lo[c], wp.bounds_hi[c] = bounds.hi[c];
  wp.info[0] = bvh.n_nodes, wp.info[1] = bvh.n_leaves, wp.info[2] = bvh.max_depth, wp.info[3] = bvh.max_leaf;
  wp.packed = bvh.packed;
  wp.has_cull = !cull.empty();
  out = std::move(wp);
  return RTW_OK;
}

}  // namespace rtwp
