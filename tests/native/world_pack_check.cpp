// The general world's device tables (csrc/rtw_world_pack.cpp, layout in
// csrc/rtw_internal.hpp "world engine") against the descriptor they were made
// from: stored order, record meta words, the BVH's shape, its child boxes
// against prim_box of every primitive beneath them, the refs packed into the
// bounds' low bytes, and the leaf pretest records.
//
// Inputs: scenes 1, 5, 6 and 7 of rtw_build_scene (7 with a procedural 64x32
// image) at flags 0, and scene 1 with RTW_WORLD_LINEAR.
//
// usage: world_pack_check [DUMP_DIR]  ->  "worlds W checks C violations V",
// exit 1 if V > 0.  With DUMP_DIR the blobs of the two BVH-free worlds are
// written there (world6.blob, world1_linear.blob) for the digest comparison.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pack_inputs.hpp"
#include "rtw_cull.hpp"
#include "rtw_layout.hpp"
#include "rtw_world_box.hpp"
#include "rtw_world_pack.hpp"

namespace {

long g_checks = 0, g_viol = 0;
const char* g_world = "";
#define CHECK(cond, ...)                               \
  do {                                                 \
    ++g_checks;                                        \
    if (!(cond) && g_viol++ < 20) {                    \
      fprintf(stderr, "%s: %s: ", g_world, #cond);     \
      fprintf(stderr, __VA_ARGS__);                    \
      fprintf(stderr, "\n");                           \
    }                                                  \
  } while (0)

template <typename T>
bool same_bits(T a, T b) {
  return std::memcmp(&a, &b, sizeof(T)) == 0;
}

struct Walk {
  const rtw_world_desc* d;
  const rtwp::WorldPack* k;
  const float* nodes;
  const float* cull;
  std::vector<uint32_t> list_of;  // stored position -> list index
  std::vector<uint32_t> in_leaves, node_seen;
  uint32_t leaves = 0, depth = 0, max_leaf = 0, cull_leaves = 0;
  double cmax_need = 0.0, rho_need = 1.0;

  Box box_of(uint32_t pos) const {
    const rtw_prim& p = d->prims[list_of[pos]];
    return prim_box(p, p.xform >= 0 ? &d->xforms[p.xform] : nullptr);
  }
  bool eligible(uint32_t pos) const {  // untransformed narrow sphere, static or moving over the shutter [0, 1]
    const rtw_prim& p = d->prims[list_of[pos]];
    if (p.xform >= 0 || !(std::fabs(p.a[6]) < 100.0)) return false;
    return p.kind == RTW_PRIM_SPHERE || (p.kind == RTW_PRIM_MOVING_SPHERE && p.a[7] == 0.0 && p.a[8] == 1.0);
  }
  void leaf(uint32_t ref, Box& sub) {
    const uint32_t first = ref & 0x7FFFFFu, cnt = (ref >> 23) & rtwk::kLeafCountMask;
    CHECK(first + cnt <= k->n_prims, "leaf [%u, +%u) past %u primitives", first, cnt, k->n_prims);
    if (first + cnt > k->n_prims) return;
    if (cnt) ++leaves;
    max_leaf = std::max(max_leaf, cnt);
    bool all_eligible = cnt >= 1 && cnt <= 2;
    for (uint32_t pos = first; pos < first + cnt; ++pos) {
      ++in_leaves[pos];
      sub.grow(box_of(pos));
      all_eligible = all_eligible && eligible(pos);
    }
    const bool pretested = (ref & rtwk::kCullBit) != 0;
    CHECK(!pretested || all_eligible, "kCullBit on leaf [%u, +%u) that does not qualify", first, cnt);
    // (cull_cmax within the limit: every qualifying leaf is pretested)
    CHECK(pretested || !all_eligible || !(k->cull_cmax <= rtwc::kCmaxLimit), "qualifying leaf [%u, +%u) without kCullBit",
          first, cnt);
    if (!pretested || !all_eligible) return;
    ++cull_leaves;
    for (uint32_t j = 0; j < cnt; ++j) {
      const rtw_prim& p = d->prims[list_of[first + j]];
      const float* q = cull + (size_t)16 * first + j;
      const float rf = (float)p.a[6];
      bool ok = same_bits(q[12], -(rf * rf));
      double c_inf = 0.0, d_inf = 0.0;
      for (int a = 0; a < 3; ++a) {
        const double dc = p.kind == RTW_PRIM_MOVING_SPHERE ? p.a[3 + a] - p.a[a] : 0.0;
        ok = ok && same_bits(q[2 * a], (float)p.a[a]) && same_bits(q[2 * (3 + a)], -(float)dc);
        c_inf = std::fmax(c_inf, std::fabs(p.a[a])), d_inf = std::fmax(d_inf, std::fabs(dc));
      }
      CHECK(ok, "pretest record of leaf [%u, +%u) sphere %u", first, cnt, j);
      cmax_need = std::fmax(cmax_need, c_inf + d_inf);
      rho_need = std::fmax(rho_need, 2.0 * p.a[6] * p.a[6] + 1.0);
    }
  }
  // Visits node n at `level` (the root is level 1); returns the box of every primitive beneath it.
  Box node(uint32_t n, uint32_t level) {
    Box all;
    depth = std::max(depth, level);
    if (node_seen[n]++) {
      CHECK(false, "node %u reached twice", n);
      return all;
    }
    const float* nd = nodes + (size_t)rtwk::kNodeWords * n;
    for (int c = 0; c < 2; ++c) {
      uint32_t ref;
      std::memcpy(&ref, nd + 12 + c, 4);
      Box sub;
      if (ref & rtwk::kLeafBit) {
        leaf(ref, sub);
      } else {
        CHECK(ref < k->n_nodes, "interior ref %u >= %u nodes", ref, k->n_nodes);
        if (ref >= k->n_nodes) continue;
        sub = node(ref, level + 1);
      }
      for (int a = 0; a < 3; ++a) {  // the stored child box (bounds as the kernel reads them) holds the subtree
        const float lo = nd[2 * a + c], hi = nd[6 + 2 * a + c];
        CHECK(!(sub.lo[a] <= sub.hi[a]) || ((double)lo <= sub.lo[a] && (double)hi >= sub.hi[a]),
              "node %u child %d axis %d: [%a, %a] does not hold [%a, %a]", n, c, a, lo, hi, sub.lo[a], sub.hi[a]);
      }
      if (k->packed) {  // the 24-bit ref in the low bytes of the child's three lower bounds
        uint32_t v = 0;
        for (int a = 0; a < 3; ++a) {
          uint32_t w;
          std::memcpy(&w, nd + 2 * a + c, 4);
          v |= (w & 255u) << (8 * a);
        }
        CHECK(v == rtwp::compact_ref(ref), "node %u child %d: gathered ref %x, compact_ref %x", n, c, v, rtwp::compact_ref(ref));
      }
      all.grow(sub);
    }
    return all;
  }
};

void verify(const char* name, const rtw_world_desc& d, const rtwp::WorldPack& k, bool expect_bvh) {
  g_world = name;
  const uint32_t n = d.n_prims;
  const unsigned char* b = k.blob.data();
  const size_t offs[10] = {k.o_prim, k.o_xform, k.o_tex, k.o_mat, k.o_perlin, k.o_image, k.o_pixels, k.o_node, k.o_order, k.o_cull};
  const long viol_before = g_viol;
  for (int t = 0; t < 10; ++t)
    CHECK(offs[t] % 256 == 0 && offs[t] < k.blob.size() && (t == 0 || offs[t] > offs[t - 1]), "table %d at %zu of %zu", t,
          offs[t], k.blob.size());
  CHECK(k.n_prims == n && k.n_perlins == d.n_perlins, "n_prims %u n_perlins %u", k.n_prims, k.n_perlins);
  if (g_viol != viol_before) return;  // (the reads below rely on these)
  const double* prim = reinterpret_cast<const double*>(b + k.o_prim);
  const uint32_t* order = reinterpret_cast<const uint32_t*>(b + k.o_order);
  const float* nodes = reinterpret_cast<const float*>(b + k.o_node);

  // ---- stored order <-> list order, the records' meta words
  Walk w{&d, &k, nodes, reinterpret_cast<const float*>(b + k.o_cull)};
  w.list_of.assign(n, ~0u);
  std::vector<uint32_t> seen(n, 0u);
  bool has_spheres = false, has_moving = false;
  uint32_t feat = 0;
  for (uint32_t pos = 0; pos < n; ++pos) {
    uint32_t meta[4], lane[2];
    std::memcpy(meta, prim + (size_t)rtwk::kWorldRec * pos + 14, sizeof(meta));
    std::memcpy(lane, prim + (size_t)rtwk::kWorldRec * pos + 11, sizeof(lane));
    const uint32_t li = meta[2];
    CHECK(li < n && !seen[li < n ? li : 0], "stored position %u: list index %u", pos, li);
    if (li >= n) return;
    ++seen[li];
    w.list_of[pos] = li;
    CHECK(order[li] == pos, "order[%u] = %u, stored at %u", li, order[li], pos);
    const rtw_prim& p = d.prims[li];
    CHECK(meta[0] == (p.kind | ((uint32_t)(p.xform + 1) << 8)) && meta[1] == p.mat && meta[3] == 0u,
          "meta of list index %u: %x %u", li, meta[0], meta[1]);
    CHECK(lane[0] == meta[0] && lane[1] == li, "double 11 of list index %u: %x %u", li, lane[0], lane[1]);
    has_spheres = has_spheres || p.kind <= RTW_PRIM_MOVING_SPHERE;
    has_moving = has_moving || p.kind == RTW_PRIM_MOVING_SPHERE;
    if (p.xform >= 0) feat |= 4u;
    if (p.kind >= RTW_PRIM_XY_RECT) feat |= 8u;
  }
  for (int c = 0; c < (int)rtwk::kWorldRec; ++c) CHECK(same_bits(prim[(size_t)rtwk::kWorldRec * n + c], 0.0), "prim padding record");
  for (uint32_t i = 0; i < d.n_textures; ++i) feat |= d.textures[i].kind == RTW_TEX_NOISE ? 1u : (d.textures[i].kind == RTW_TEX_IMAGE ? 2u : 0u);
  CHECK(k.feat == feat && k.has_moving == has_moving && k.view_flags == (has_spheres ? rtwk::kWorldHasSpheres : 0u),
        "feat %u (expected %u), has_moving %d, flags %u", k.feat, feat, (int)k.has_moving, k.view_flags);
  Box all;
  for (uint32_t pos = 0; pos < n; ++pos) all.grow(w.box_of(pos));
  for (int a = 0; a < 3; ++a) CHECK(same_bits(k.bounds_lo[a], all.lo[a]) && same_bits(k.bounds_hi[a], all.hi[a]), "bounds axis %d", a);
  // image table and pixel pool
  const uint32_t* img = reinterpret_cast<const uint32_t*>(b + k.o_image);
  size_t pix = 0;
  for (uint32_t i = 0; i < d.n_images; ++i) {
    const size_t bytes = (size_t)d.images[i].width * d.images[i].height * 4;
    CHECK(img[4 * i] == d.images[i].width && img[4 * i + 1] == d.images[i].height && img[4 * i + 2] == (uint32_t)pix &&
              img[4 * i + 3] == (uint32_t)(pix >> 32),
          "image record %u", i);
    CHECK(k.o_pixels + pix + bytes <= k.o_node && std::memcmp(b + k.o_pixels + pix, d.images[i].rgba, bytes) == 0,
          "pixels of image %u", i);
    pix += bytes;
  }

  // ---- BVH
  CHECK((k.n_nodes > 0) == expect_bvh && k.info[0] == k.n_nodes, "%u nodes (info %u), BVH expected: %d", k.n_nodes, k.info[0],
        (int)expect_bvh);
  CHECK(k.o_node + ((size_t)k.n_nodes + 2) * rtwk::kNodeWords * 4 <= k.o_order, "node table overruns");
  for (uint32_t i = 0; i < 2 * rtwk::kNodeWords; ++i)
    CHECK(same_bits(nodes[(size_t)rtwk::kNodeWords * k.n_nodes + i], 0.0f), "node padding word %u", i);
  if (!k.n_nodes) {
    for (uint32_t pos = 0; pos < n; ++pos) CHECK(w.list_of[pos] == pos, "BVH-free world: position %u holds list index %u", pos, w.list_of[pos]);
    CHECK(!k.packed && k.info[1] == 0 && k.info[2] == 0 && k.info[3] == 0, "BVH-free world: info / packed");
    return;
  }
  w.in_leaves.assign(n, 0u);
  w.node_seen.assign(k.n_nodes, 0u);
  w.node(0, 1);
  for (uint32_t pos = 0; pos < n; ++pos) CHECK(w.in_leaves[pos] == 1u, "stored position %u lies in %u leaf ranges", pos, w.in_leaves[pos]);
  for (uint32_t i = 0; i < k.n_nodes; ++i) CHECK(w.node_seen[i] == 1u, "node %u reached %u times", i, w.node_seen[i]);
  CHECK(k.info[1] == w.leaves && k.info[2] == w.depth && k.info[3] == w.max_leaf, "info %u leaves, depth %u, max leaf %u; walked %u, %u, %u",
        k.info[1], k.info[2], k.info[3], w.leaves, w.depth, w.max_leaf);
  CHECK(w.depth <= (w.max_leaf == 1 ? rtwk::kLaneStack : rtwk::kBvhStack - 1), "depth %u with leaves of <= %u", w.depth, w.max_leaf);
  CHECK(k.packed, "refs not packed (%u nodes, %u primitives, max leaf %u)", k.n_nodes, n, w.max_leaf);
  if (has_spheres) CHECK(w.cull_leaves > 0, "no leaf is pretested");
  if (w.cull_leaves)
    CHECK((double)k.cull_cmax >= w.cmax_need && (double)k.cull_rho >= w.rho_need, "cull_cmax %a < %a or cull_rho %a < %a",
          k.cull_cmax, w.cmax_need, k.cull_rho, w.rho_need);
}

int g_worlds = 0;
void run(const char* name, uint32_t scene, uint32_t flags, bool expect_bvh, const char* dump_dir) {
  g_world = name;
  ++g_worlds;
  const std::vector<uint8_t> px = pack_inputs::procedural_image(64, 32);
  const rtw_image image{64, 32, px.data()};
  rtw_built_scene built = nullptr;
  rtw_world_desc d;
  rtw_scene_settings settings;
  const bool made = rtw_build_scene(scene, 42, &image, &built) == RTW_OK && rtw_built_scene_desc(built, &d, &settings, nullptr) == RTW_OK;
  CHECK(made, "rtw_build_scene(%u) failed", scene);
  if (!made) return;
  rtwp::WorldPack k;
  std::string msg;
  const int st = rtwp::pack_world(&d, flags, false, k, msg);
  CHECK(st == RTW_OK, "pack_world: %d %s", st, msg.c_str());
  if (st == RTW_OK) {
    verify(name, d, k, expect_bvh);
    if (dump_dir) {
      FILE* f = fopen((std::string(dump_dir) + "/" + name + ".blob").c_str(), "wb");
      if (!f || fwrite(k.blob.data(), 1, k.blob.size(), f) != k.blob.size()) CHECK(false, "cannot write the blob");
      if (f) fclose(f);
    }
  }
  rtw_built_scene_free(built);
}

}  // namespace

int main(int argc, char** argv) {
  const char* dump_dir = argc > 1 ? argv[1] : nullptr;
  run("world1", 1, 0, true, nullptr);
  run("world5", 5, 0, false, nullptr);
  run("world6", 6, 0, false, dump_dir);
  run("world7", 7, 0, true, nullptr);
  run("world1_linear", 1, RTW_WORLD_LINEAR, false, dump_dir);
  printf("worlds %d checks %ld violations %ld\n", g_worlds, g_checks, g_viol);
  return g_viol ? 1 : 0;
}
