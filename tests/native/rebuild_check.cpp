// The host rebuild of a dynamic world's tree (csrc/rtw_world_build.cpp, the
// per-item functions of csrc/rtw_world_build.hpp that the rebuild kernels run
// too) against the descriptor and against statements made here a second time:
//   1. need_of / cap_of / split_of at counts 1, 2, 3, 2^k, 2^k + 1 and at keys
//      that differ only in bit 0 or only in bit 62; spread3 against a loop;
//   2. per world, after rebuild_world + refit_world of its own numbers: n - 1
//      nodes, the root is record 0, the numbering is breadth-first (interior
//      children only, child 0 first), every leaf holds one primitive and every
//      primitive is in exactly one leaf; depth <= cap and d + need <= cap at
//      every node; info[2] is the depth; every split is where a linear scan of
//      the keys (computed here from the packer's prim_box) puts it; the stored
//      order is the stable sort by key; order is a permutation and each
//      record's meta and numbers match its list index; every child box holds
//      the packer's f64 box of each primitive beneath it; the packed lower
//      bounds decode to compact_ref(ref); the refit's schedule never puts a
//      child at or after its parent; candidates and mates follow eligibility;
//   3. the same tree from a shuffled description, indices mapped back (where
//      keys tie, the same set of primitives);
//   4. given a second file of the same world with other numbers (a1):
//      rebuild(a0) + refit(a1) and rebuild(a1) + refit(a1) agree in the world
//      box, cull_cmax, cull_rho, every primitive's leaf box and the root box;
//      and a rebuild is idempotent: rebuild(a1) twice gives the same bytes,
//      from the created tables or from the tables of rebuild(a0).
//
// usage: rebuild_check WORLD.bin[:MOVED.bin]...  (descriptors dumped by tests/test_rebuild_host.py)
//   ->  "worlds W checks C violations V", exit 1 if V > 0.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "rtw_layout.hpp"
#include "rtw_world_box.hpp"
#include "rtw_world_build.hpp"
#include "rtw_world_pack.hpp"
#include "rtw_world_refit.hpp"

namespace {

long g_checks = 0, g_viol = 0;
std::string g_world;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    ++g_checks;                                            \
    if (!(cond) && g_viol++ < 20) {                        \
      fprintf(stderr, "%s: %s: ", g_world.c_str(), #cond); \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n");                               \
    }                                                      \
  } while (0)

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

struct World {
  std::vector<rtw_prim> prims;
  std::vector<rtw_xform> xforms;
  std::vector<rtw_texture> tex;
  std::vector<rtw_wmaterial> mats;
  std::vector<rtw_perlin> perl;
  std::vector<rtw_image> images;
  std::vector<std::vector<uint8_t>> pixels;
  uint32_t flags = 0;
  rtw_world_desc desc() const {
    rtw_world_desc d;
    d.prims = prims.data(), d.n_prims = (uint32_t)prims.size();
    d.xforms = xforms.data(), d.n_xforms = (uint32_t)xforms.size();
    d.textures = tex.data(), d.n_textures = (uint32_t)tex.size();
    d.mats = mats.data(), d.n_mats = (uint32_t)mats.size();
    d.perlins = perl.data(), d.n_perlins = (uint32_t)perl.size();
    d.images = images.data(), d.n_images = (uint32_t)images.size();
    return d;
  }
  void numbers(std::vector<double>& a, std::vector<double>& xv) const {
    a.resize(9 * prims.size()), xv.resize(12 * xforms.size());
    for (size_t i = 0; i < prims.size(); ++i) std::memcpy(&a[9 * i], prims[i].a, sizeof(prims[i].a));
    for (size_t i = 0; i < xforms.size(); ++i) std::memcpy(&xv[12 * i], xforms[i].v, sizeof(xforms[i].v));
  }
};

template <typename T>
bool read_vec(FILE* f, std::vector<T>& v) {
  uint32_t n = 0;
  if (fread(&n, 4, 1, f) != 1) return false;
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
bool load(const char* path, World& w) {  // tests/update_helpers.py dump_desc
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  bool ok = fread(&w.flags, 4, 1, f) == 1 && read_vec(f, w.prims) && read_vec(f, w.xforms) && read_vec(f, w.tex) &&
            read_vec(f, w.mats) && read_vec(f, w.perl);
  uint32_t n_img = 0;
  ok = ok && fread(&n_img, 4, 1, f) == 1;
  for (uint32_t i = 0; ok && i < n_img; ++i) {
    uint32_t wh[2];
    ok = fread(wh, 4, 2, f) == 2;
    if (!ok) break;
    w.pixels.emplace_back((size_t)wh[0] * wh[1] * 4);
    ok = fread(w.pixels.back().data(), 1, w.pixels.back().size(), f) == w.pixels.back().size();
    w.images.push_back(rtw_image{wh[0], wh[1], nullptr});
  }
  for (size_t i = 0; i < w.images.size(); ++i) w.images[i].rgba = w.pixels[i].data();
  fclose(f);
  return ok;
}

// ------------------------------------------------------------ 1. the pieces --
uint32_t ceil_log2(uint32_t c) {
  uint32_t k = 0;
  while ((1ull << k) < c) ++k;
  return k;
}
uint64_t spread_loop(uint64_t v) {
  uint64_t r = 0;
  for (int i = 0; i < 21; ++i) r |= ((v >> i) & 1ull) << (3 * i);
  return r;
}
// the split as a linear scan states it
uint32_t split_scan(const std::vector<uint64_t>& keys, uint32_t b, uint32_t e, uint32_t d, uint32_t cap) {
  const uint32_t mid = b + (e - b) / 2;
  if (d + ceil_log2(e - b) >= cap || keys[b] == keys[e - 1]) return mid;
  int p = 62;
  while (((keys[b] ^ keys[e - 1]) >> p) == 0) --p;
  for (uint32_t i = b + 1; i < e; ++i)
    if ((keys[i] >> p) & 1ull) return i;
  return e;
}

void check_pieces() {
  g_world = "pieces";
  std::vector<uint32_t> counts = {1, 2, 3};
  for (uint32_t k = 2; k <= 23; ++k) counts.push_back(1u << k), counts.push_back((1u << k) + 1u);
  for (uint32_t c : counts) CHECK(rtwb::need_of(c) == ceil_log2(c), "need_of(%u) = %u", c, rtwb::need_of(c));
  CHECK(rtwb::cap_of(1u << 16) == rtwk::kLaneStack && rtwb::cap_of((1u << 16) + 1) == rtwk::kBvhStack - 1, "cap_of");
  CHECK(rtwb::cap_of(600) == rtwk::kLaneStack, "cap_of(600)");
  Rng g{3};
  for (int i = 0; i < 2000; ++i) {
    const uint64_t v = g.next() & 0x1FFFFF;
    CHECK(rtwb::spread3(v) == spread_loop(v), "spread3(%llx)", (unsigned long long)v);
  }
  CHECK(rtwb::spread3(0x1FFFFF) == 0x1249249249249249ull, "spread3 of all ones");
  CHECK(rtwb::key_field(1.0, 0.0, 1.0) == 2097151u && rtwb::key_field(0.0, 0.0, 1.0) == 0u &&
            rtwb::key_field(5.0, 5.0, 0.0) == 0u && rtwb::key_field(0.5, 0.0, 1.0) == 1048576u,
        "key_field edges");
  const double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1}, cx[3] = {1, 0, 0}, cz[3] = {0, 0, 1};
  CHECK(rtwb::morton_key(cx, lo, hi) == (0x1249249249249249ull << 2) && rtwb::morton_key(cz, lo, hi) == 0x1249249249249249ull,
        "x is the highest field, z the lowest");
  // splits: small counts, powers of two and their successors, with a deep and a shallow cap
  for (uint32_t c : counts) {
    if (c < 2 || c > (1u << 12) + 1) continue;
    for (int pattern = 0; pattern < 5; ++pattern) {
      std::vector<uint64_t> keys(c);
      const uint32_t flip = 1 + (uint32_t)(g.next() % (c - 1));  // the first index of the upper part
      for (uint32_t i = 0; i < c; ++i) {
        if (pattern == 0) keys[i] = 77;                                  // all equal: the median
        else if (pattern == 1) keys[i] = 76 | (i >= flip ? 1ull : 0ull);  // differ only in bit 0
        else if (pattern == 2) keys[i] = 5 | (i >= flip ? 1ull << 62 : 0ull);  // differ only in bit 62
        else if (pattern == 3) keys[i] = i;
        else keys[i] = g.next() >> 1;
      }
      if (pattern == 4) std::sort(keys.begin(), keys.end());
      for (uint32_t d : {0u, 3u, 15u}) {
        const uint32_t cap = rtwk::kLaneStack;
        if (d + ceil_log2(c) > cap) continue;
        const uint32_t m = rtwb::split_of(keys.data(), 0, c, d, cap), want = split_scan(keys, 0, c, d, cap);
        CHECK(m == want && m > 0 && m < c, "count %u pattern %d depth %u: split %u, scan %u", c, pattern, d, m, want);
        if ((pattern == 1 || pattern == 2) && d + ceil_log2(c) < cap) CHECK(m == flip, "count %u: split %u, bit flips at %u", c, m, flip);
        if (pattern == 0 || d + ceil_log2(c) >= cap) CHECK(m == c / 2, "count %u depth %u: median", c, d);
      }
    }
  }
}

// -------------------------------------------------------------- 2. a world --
struct Built {
  rtwp::WorldPack k;
  rtwp::RefitPack r;
  const float* nodes() const { return reinterpret_cast<const float*>(k.blob.data() + k.o_node); }
  const float* plain() const { return reinterpret_cast<const float*>(r.blob.data() + r.o_plain); }
  const double* prim() const { return reinterpret_cast<const double*>(k.blob.data() + k.o_prim); }
  const uint32_t* order() const { return reinterpret_cast<const uint32_t*>(k.blob.data() + k.o_order); }
  uint32_t ref(uint32_t n, int c) const { return rtwr::ld_u32(nodes() + (size_t)rtwk::kNodeWords * n, 12 + c); }
};

bool create(const World& w, Built& t) {
  rtw_world_desc d = w.desc();
  std::string msg;
  if (rtwp::pack_world(&d, w.flags, false, t.k, msg) != RTW_OK) {
    fprintf(stderr, "%s: pack_world: %s\n", g_world.c_str(), msg.c_str());
    return false;
  }
  rtwp::make_refit(&d, t.k, t.r);
  return true;
}
bool rebuild(Built& t, const std::vector<double>& a, const std::vector<double>& xv) {
  const double* xp = xv.empty() ? nullptr : xv.data();
  const int s1 = rtwp::rebuild_world(t.k, t.r, a.data(), xp);
  const int s2 = s1 == RTW_OK ? rtwp::refit_world(t.k, t.r, a.data(), xp) : s1;
  CHECK(s1 == RTW_OK && s2 == RTW_OK, "rebuild %d refit %d: %s", s1, s2, t.r.msg.c_str());
  return s1 == RTW_OK && s2 == RTW_OK;
}

// keys from the packer's own prim_box (rtw_world_box.hpp), stated a second time
std::vector<uint64_t> keys_of(const World& w) {
  const size_t n = w.prims.size();
  std::vector<std::array<double, 3>> c(n);
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (size_t i = 0; i < n; ++i) {
    const rtw_prim& p = w.prims[i];
    const Box b = ::prim_box(p, p.xform >= 0 ? &w.xforms[p.xform] : nullptr);
    for (int k = 0; k < 3; ++k) c[i][k] = 0.5 * (b.lo[k] + b.hi[k]), lo[k] = std::min(lo[k], c[i][k]), hi[k] = std::max(hi[k], c[i][k]);
  }
  std::vector<uint64_t> key(n);
  for (size_t i = 0; i < n; ++i) {
    uint64_t f[3];
    for (int k = 0; k < 3; ++k) {
      const double ext = hi[k] - lo[k];
      f[k] = ext == 0.0 ? 0u : std::min<uint64_t>(2097151u, (uint64_t)((c[i][k] - lo[k]) / ext * 2097152.0));
    }
    key[i] = (spread_loop(f[0]) << 2) | (spread_loop(f[1]) << 1) | spread_loop(f[2]);
  }
  return key;
}

struct NodeInfo {
  uint32_t b = 0, e = 0, depth = 0;
};

void verify(const World& w, const Built& t, const rtwp::WorldPack& created) {
  const uint32_t n = (uint32_t)w.prims.size(), nn = t.k.n_nodes, cap = rtwb::cap_of(n);
  CHECK(nn == n - 1 && t.k.info[0] == nn && t.k.info[1] == n && t.k.info[3] == 1, "%u nodes for %u primitives", nn, n);
  CHECK(t.k.blob.size() == created.blob.size() && t.k.packed == created.packed && t.k.has_cull == created.has_cull, "sizes");
  // order: a permutation; records: meta and numbers of their list index
  std::vector<uint32_t> list_of(n, ~0u);
  for (uint32_t li = 0; li < n; ++li) {
    const uint32_t pos = t.order()[li];
    CHECK(pos < n && list_of[pos] == ~0u, "order[%u] = %u", li, pos);
    if (pos >= n) return;
    list_of[pos] = li;
    const double* rec = t.prim() + (size_t)rtwk::kWorldRec * pos;
    const rtw_prim& p = w.prims[li];
    const uint32_t meta0 = p.kind | ((uint32_t)(p.xform + 1) << 8);
    CHECK(rtwr::ld_u32(rec + 14, 0) == meta0 && rtwr::ld_u32(rec + 14, 1) == p.mat && rtwr::ld_u32(rec + 14, 2) == li &&
              rtwr::ld_u32(rec + 14, 3) == 0u && rtwr::ld_u32(rec + 11, 0) == meta0 && rtwr::ld_u32(rec + 11, 1) == li,
          "meta of list index %u at %u", li, pos);
    double want[11];
    rtwr::fill_record(p.kind, p.a, want);
    CHECK(std::memcmp(rec, want, sizeof(want)) == 0, "numbers of list index %u", li);
  }
  // the stored order is the stable sort by key
  const std::vector<uint64_t> key = keys_of(w);
  std::vector<uint64_t> keys(n);
  for (uint32_t pos = 0; pos < n; ++pos) keys[pos] = key[list_of[pos]];
  for (uint32_t pos = 1; pos < n; ++pos)
    CHECK(keys[pos - 1] < keys[pos] || (keys[pos - 1] == keys[pos] && list_of[pos - 1] < list_of[pos]), "sorted at %u", pos);
  // topology, breadth-first from the root
  std::vector<NodeInfo> info(nn);
  std::vector<uint32_t> seen(n, 0u), level_of(nn, 0u);
  info[0].b = 0, info[0].e = n;
  uint32_t next = 1, depth = 0;
  for (uint32_t x = 0; x < nn; ++x) {
    CHECK(x < next, "node %u is reached from the root", x);
    if (x >= next) return;
    const NodeInfo ni = info[x];
    depth = std::max(depth, ni.depth + 1);
    CHECK(ni.e - ni.b >= 2 && ni.depth + ceil_log2(ni.e - ni.b) <= cap, "node %u: depth %u, %u primitives, cap %u", x, ni.depth,
          ni.e - ni.b, cap);
    const uint32_t m = split_scan(keys, ni.b, ni.e, ni.depth, cap);
    const uint32_t cb[2] = {ni.b, m}, ce[2] = {m, ni.e};
    for (int c = 0; c < 2; ++c) {
      const uint32_t ref = t.ref(x, c);
      if (ce[c] - cb[c] == 1) {
        CHECK((ref & ~rtwk::kCullBit) == (rtwk::kLeafBit | (1u << 23) | cb[c]), "node %u child %d: ref %08x, leaf of %u", x, c, ref, cb[c]);
        if (cb[c] < n) seen[cb[c]]++;
      } else {
        CHECK(ref == next, "node %u child %d: ref %08x, breadth-first %u", x, c, ref, next);
        if (next < nn) info[next].b = cb[c], info[next].e = ce[c], info[next].depth = ni.depth + 1;
        ++next;
      }
      // packed lower bounds carry the ref
      if (t.k.packed) {
        const float* nd = t.nodes() + (size_t)rtwk::kNodeWords * x;
        uint32_t v = 0;
        for (int k = 0; k < 3; ++k) v |= (rtwr::f32_bits(nd[2 * k + c]) & 255u) << (8 * k);
        CHECK(v == rtwr::compact_ref(ref & ~rtwk::kCullBit), "node %u child %d: packed %06x", x, c, v);
      }
    }
  }
  CHECK(next == nn, "%u nodes numbered, %u records", next, nn);
  for (uint32_t pos = 0; pos < n; ++pos) CHECK(seen[pos] == 1, "position %u is in %u leaves", pos, seen[pos]);
  CHECK(depth <= cap && t.k.info[2] == depth, "depth %u, info %u, cap %u", depth, t.k.info[2], cap);
  // boxes: every child box holds the packer's f64 box of each primitive beneath it
  std::vector<Box> pbox(n);
  for (uint32_t pos = 0; pos < n; ++pos) {
    const rtw_prim& p = w.prims[list_of[pos]];
    pbox[pos] = ::prim_box(p, p.xform >= 0 ? &w.xforms[p.xform] : nullptr);
  }
  for (uint32_t x = 0; x < nn; ++x) {
    const uint32_t m = split_scan(keys, info[x].b, info[x].e, info[x].depth, cap);
    const uint32_t cb[2] = {info[x].b, m}, ce[2] = {m, info[x].e};
    const float *nd = t.nodes() + (size_t)rtwk::kNodeWords * x, *pl = t.plain() + (size_t)12 * x;
    for (int c = 0; c < 2; ++c) {
      Box u;
      for (uint32_t pos = cb[c]; pos < ce[c]; ++pos) u.grow(pbox[pos]);
      for (int k = 0; k < 3; ++k) {
        CHECK((double)pl[2 * k + c] <= u.lo[k] && (double)pl[6 + 2 * k + c] >= u.hi[k], "node %u child %d axis %d: plain box", x, c, k);
        CHECK(nd[2 * k + c] <= pl[2 * k + c] && nd[6 + 2 * k + c] == pl[6 + 2 * k + c], "node %u child %d axis %d: node box", x, c, k);
        // tight: the plain bounds are the outward roundings of the union
        CHECK(pl[2 * k + c] == rtwr::down(u.lo[k]) && pl[6 + 2 * k + c] == rtwr::up(u.hi[k]), "node %u child %d axis %d: tight", x, c, k);
      }
    }
  }
  // the refit's schedule: a permutation of the nodes in which every interior child comes before its parent,
  // with a smaller label; launches are per label
  const uint32_t* by_height = reinterpret_cast<const uint32_t*>(t.r.blob.data() + t.r.o_by_height);
  const uint32_t* heights = reinterpret_cast<const uint32_t*>(t.r.blob.data() + t.r.o_heights);
  const uint32_t* cand = reinterpret_cast<const uint32_t*>(t.r.blob.data() + t.r.o_cand);
  const uint32_t* mate = reinterpret_cast<const uint32_t*>(t.r.blob.data() + t.r.o_mate);
  std::vector<uint32_t> label(nn, 0u);
  for (uint32_t i = 0; i < nn; ++i) {
    CHECK(by_height[i] < nn && label[by_height[i]] == 0u && heights[i] >= 1 && heights[i] <= t.r.h_max, "schedule entry %u", i);
    if (by_height[i] < nn) label[by_height[i]] = heights[i];
    if (i) CHECK(heights[i - 1] <= heights[i], "labels ascend at %u", i);
    CHECK(i >= t.r.h_off[heights[i] - 1] && i < t.r.h_off[heights[i]], "entry %u lies in its label's range", i);
  }
  CHECK(t.r.h_max == depth && t.r.h_off[depth] == nn && nn - t.r.h_off[t.r.h_star - 1] <= rtwr::kBlock, "h_max %u h_star %u", t.r.h_max, t.r.h_star);
  for (uint32_t x = 0; x < nn; ++x)
    for (int c = 0; c < 2; ++c) {
      const uint32_t ref = t.ref(x, c);
      if (!(ref & rtwk::kLeafBit)) CHECK(label[ref] < label[x], "node %u (label %u) child %u (label %u)", x, label[x], ref, label[ref]);
      else {
        const uint32_t pos = ref & 0x7FFFFFu, li = list_of[pos];
        const rtw_prim& p = w.prims[li];
        const bool el = rtwr::eligible(p.kind | ((uint32_t)(p.xform + 1) << 8), p.a);
        CHECK((((cand[x] >> c) & 1u) != 0u) == el && mate[li] == (el ? li : rtwr::kNone), "candidate: node %u child %d", x, c);
        CHECK(!(ref & rtwk::kCullBit) || (el && t.k.has_cull), "node %u child %d: pretest bit", x, c);
      }
    }
}

// ---------------------------------------------------------- 3. shuffled ----
void check_shuffled(const World& w, const Built& t) {
  const uint32_t n = (uint32_t)w.prims.size();
  std::vector<uint32_t> perm(n);
  std::iota(perm.begin(), perm.end(), 0u);
  Rng g{n};
  for (uint32_t i = n - 1; i > 0; --i) std::swap(perm[i], perm[g.next() % (i + 1)]);
  World s = w;
  for (uint32_t i = 0; i < n; ++i) s.prims[i] = w.prims[perm[i]];  // shuffled index i holds list index perm[i]
  Built u;
  std::vector<double> a, xv;
  s.numbers(a, xv);
  if (!create(s, u) || !rebuild(u, a, xv)) return;
  const std::vector<uint64_t> key = keys_of(w);
  std::vector<uint32_t> list_t(n), list_u(n);
  for (uint32_t li = 0; li < n; ++li) list_t[t.order()[li]] = li, list_u[u.order()[li]] = perm[li];
  CHECK(u.k.info[2] == t.k.info[2], "shuffled: depth %u against %u", u.k.info[2], t.k.info[2]);
  for (uint32_t x = 0; x < t.k.n_nodes; ++x)
    for (int c = 0; c < 2; ++c)
      CHECK((u.ref(x, c) & ~rtwk::kCullBit) == (t.ref(x, c) & ~rtwk::kCullBit), "shuffled: node %u child %d", x, c);
  for (uint32_t b = 0; b < n;) {  // runs of equal keys hold the same primitives; a run of one, the same primitive
    uint32_t e = b + 1;
    while (e < n && key[list_t[e]] == key[list_t[b]]) ++e;
    std::vector<uint32_t> x(list_t.begin() + b, list_t.begin() + e), y(list_u.begin() + b, list_u.begin() + e);
    std::sort(x.begin(), x.end()), std::sort(y.begin(), y.end());
    CHECK(x == y, "shuffled: positions %u .. %u", b, e);
    b = e;
  }
}

// -------------------------------------------------- 4. rebuild and refit ----
void check_moved(const World& w0, const World& w1) {
  std::vector<double> a0, xv0, a1, xv1;
  w0.numbers(a0, xv0), w1.numbers(a1, xv1);
  const double* xp1 = xv1.empty() ? nullptr : xv1.data();
  Built p, q, s;
  if (!create(w0, p) || !create(w0, q) || !create(w0, s)) return;
  // p: rebuild(a0), refit(a1).  q: rebuild(a1) (+ its identity refit).  s: rebuild(a0), rebuild(a1).
  if (!rebuild(p, a0, xv0) || !rebuild(q, a1, xv1) || !rebuild(s, a0, xv0) || !rebuild(s, a1, xv1)) return;
  CHECK(rtwp::refit_world(p.k, p.r, a1.data(), xp1) == RTW_OK, "refit of the moved numbers");
  const rtwp::WorldPack q0 = q.k;
  CHECK(rtwp::refit_world(q.k, q.r, a1.data(), xp1) == RTW_OK && q.k.blob == q0.blob, "an identity refit changes nothing");
  CHECK(s.k.blob == q.k.blob && std::memcmp(s.k.info, q.k.info, sizeof(q.k.info)) == 0 &&
            rtwr::f32_bits(s.k.cull_cmax) == rtwr::f32_bits(q.k.cull_cmax) && rtwr::f32_bits(s.k.cull_rho) == rtwr::f32_bits(q.k.cull_rho) &&
            std::memcmp(s.k.bounds_lo, q.k.bounds_lo, 24) == 0 && std::memcmp(s.k.bounds_hi, q.k.bounds_hi, 24) == 0,
        "a rebuild does not depend on the tables it starts from");
  CHECK(std::memcmp(p.k.bounds_lo, q.k.bounds_lo, 24) == 0 && std::memcmp(p.k.bounds_hi, q.k.bounds_hi, 24) == 0, "world box");
  CHECK(rtwr::f32_bits(p.k.cull_cmax) == rtwr::f32_bits(q.k.cull_cmax) && rtwr::f32_bits(p.k.cull_rho) == rtwr::f32_bits(q.k.cull_rho),
        "cull scalars %g %g against %g %g", p.k.cull_cmax, p.k.cull_rho, q.k.cull_cmax, q.k.cull_rho);
  // every primitive's leaf box, and the root box
  const uint32_t n = (uint32_t)w0.prims.size();
  auto leaf_boxes = [&](const Built& t, std::vector<float>& out, float root[6]) {
    out.assign((size_t)6 * n, 0.0f);
    std::vector<uint32_t> list_of(n);
    for (uint32_t li = 0; li < n; ++li) list_of[t.order()[li]] = li;
    for (uint32_t x = 0; x < t.k.n_nodes; ++x)
      for (int c = 0; c < 2; ++c)
        if (t.ref(x, c) & rtwk::kLeafBit)
          for (int k = 0; k < 6; ++k) out[(size_t)6 * list_of[t.ref(x, c) & 0x7FFFFFu] + k] = t.plain()[(size_t)12 * x + 2 * k + c];
    for (int k = 0; k < 3; ++k)
      root[k] = rtwr::fmin32(t.plain()[2 * k], t.plain()[2 * k + 1]), root[3 + k] = rtwr::fmax32(t.plain()[6 + 2 * k], t.plain()[7 + 2 * k]);
  };
  std::vector<float> bp, bq;
  float rp[6], rq[6];
  leaf_boxes(p, bp, rp), leaf_boxes(q, bq, rq);
  CHECK(std::memcmp(bp.data(), bq.data(), bp.size() * 4) == 0, "leaf boxes");
  CHECK(std::memcmp(rp, rq, sizeof(rp)) == 0, "root box");
  g_checks += 6 * n;
}

}  // namespace

int main(int argc, char** argv) {
  check_pieces();
  int worlds = 0;
  for (int i = 1; i < argc; ++i) {
    std::string arg = argv[i], moved;
    const size_t colon = arg.find(':');
    if (colon != std::string::npos) moved = arg.substr(colon + 1), arg = arg.substr(0, colon);
    World w;
    g_world = arg;
    if (!load(arg.c_str(), w)) {
      fprintf(stderr, "cannot read %s\n", arg.c_str());
      return 2;
    }
    Built created, t;
    std::vector<double> a, xv;
    w.numbers(a, xv);
    if (!create(w, created) || !create(w, t)) return 2;
    // a refused rebuild leaves the tables as they were
    std::vector<double> bad = a;
    bad[9 * (a.size() / 18) + 1] = NAN;
    CHECK(rtwp::rebuild_world(t.k, t.r, bad.data(), xv.empty() ? nullptr : xv.data()) == RTW_EINVAL && t.k.blob == created.k.blob &&
              t.r.blob == created.r.blob && t.k.info[2] == created.k.info[2],
          "a refused rebuild");
    if (rebuild(t, a, xv)) {
      verify(w, t, created.k);
      check_shuffled(w, t);
    }
    if (!moved.empty()) {
      World w1;
      g_world = moved;
      if (!load(moved.c_str(), w1) || w1.prims.size() != w.prims.size()) {
        fprintf(stderr, "cannot read %s\n", moved.c_str());
        return 2;
      }
      Built t1;
      std::vector<double> a1, xv1;
      w1.numbers(a1, xv1);
      if (create(w, t1) && rebuild(t1, a1, xv1)) {
        verify(w1, t1, created.k);
        check_shuffled(w1, t1);
      }
      check_moved(w, w1);
    }
    ++worlds;
  }
  printf("worlds %d checks %ld violations %ld\n", worlds, g_checks, g_viol);
  return g_viol ? 1 : 0;
}
