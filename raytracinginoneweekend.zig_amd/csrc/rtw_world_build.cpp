// rtw_world_build.cpp — the host rebuild of a dynamic world's tree (rtw_hip.h
// rtw_world_rebuild): the definition of what a rebuild leaves in
// the tables before the refit's commit runs over the new tree.  The kernels
// (rtw_world_rebuild.hip) run the same per-item functions
// (rtw_world_build.hpp), so the device tables equal these byte for byte.
// Plain C++: no HIP, no environment.
#include <algorithm>
#include <cassert>
#include <cstring>
#include <numeric>

#include "rtw_layout.hpp"
#include "rtw_world_build.hpp"
#include "rtw_world_pack.hpp"
#include "rtw_tri.hpp"
#include "rtw_world_refit.hpp"

namespace rtwp {

bool rebuild_supported(uint32_t n_prims, uint32_t n_nodes, const uint32_t info[4]) {
  return n_nodes > 0 && info[3] == 1u && n_prims >= 2u && n_nodes == n_prims - 1u;
}

void level_schedule(const uint32_t* level_count, uint32_t depth, uint32_t n_nodes, RefitPack& r) {
  // label h = depth - level: h_off[h] = nodes of the levels depth - h and deeper
  r.h_max = depth;
  r.h_off.assign(depth + 1, 0u);
  for (uint32_t h = 1; h <= depth; ++h) r.h_off[h] = r.h_off[h - 1] + level_count[depth - h];
  assert(r.h_off[depth] == n_nodes);
  r.h_star = 1;
  while (r.h_star < r.h_max && n_nodes - r.h_off[r.h_star - 1] > rtwr::kBlock) ++r.h_star;
}

int rebuild_world(WorldPack& k, RefitPack& r, const double* a, const double* xv) {
  const uint32_t n = k.n_prims, nn = k.n_nodes;
  if (!rebuild_supported(n, nn, k.info)) {
    r.msg = "rebuild: the world has no BVH with leaves of one primitive";
    return RTW_UNSUPPORTED;
  }
  unsigned char* b = k.blob.data();
  unsigned char* rb = r.blob.data();
  double* prim = reinterpret_cast<double*>(b + k.o_prim);
  float* node = reinterpret_cast<float*>(b + k.o_node);
  uint32_t* order = reinterpret_cast<uint32_t*>(b + k.o_order);
  float* cull = reinterpret_cast<float*>(b + k.o_cull);
  uint32_t* by_height = reinterpret_cast<uint32_t*>(rb + r.o_by_height);
  uint32_t* heights = reinterpret_cast<uint32_t*>(rb + r.o_heights);
  uint32_t* cand = reinterpret_cast<uint32_t*>(rb + r.o_cand);
  uint32_t* mate = reinterpret_cast<uint32_t*>(rb + r.o_mate);

  // validate: a leaf of one is judged on its own sphere, so every primitive is its own mate
  rtwr::View V = refit_view(k, r, a, xv);
  std::vector<uint32_t> self(n);
  std::iota(self.begin(), self.end(), 0u);
  V.mate = self.data();
  rtwr::Partial p;
  rtwr::partial_init(p);
  for (uint32_t i = 0; i < n; ++i) rtwr::validate_prim(V, i, p);
  for (uint32_t i = 0; i < V.n_xforms; ++i) rtwr::validate_xform(V, i, p);
  if (p.bad != 0.0) {
    r.msg = refit_violation(p.bad, p.first_bad, n);
    return RTW_EINVAL;
  }

  // keys: the centroid box (total order on zeros), then a Morton code per primitive
  double clo[3] = {rtwr::inf(), rtwr::inf(), rtwr::inf()}, chi[3] = {-rtwr::inf(), -rtwr::inf(), -rtwr::inf()};
  for (uint32_t i = 0; i < n; ++i) {
    double lo[3], hi[3], c[3];
    rtwr::box_of(V, rtwr::prim_meta0(V, V.order[i]), i, lo, hi);
    rtwb::centroid(lo, hi, c);
    for (int x = 0; x < 3; ++x) clo[x] = rtwr::tmin(clo[x], c[x]), chi[x] = rtwr::tmax(chi[x], c[x]);
  }
  std::vector<uint64_t> key(n), keys(n);
  for (uint32_t i = 0; i < n; ++i) key[i] = rtwb::key_of(V, i, clo, chi);
  std::vector<uint32_t> sorted(n);  // new stored position -> list index
  std::iota(sorted.begin(), sorted.end(), 0u);
  std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
  for (uint32_t pos = 0; pos < n; ++pos) keys[pos] = key[sorted[pos]];

  // topology: level by level, interior children numbered left to right behind the level
  const uint32_t cap = rtwb::cap_of(n);
  std::vector<uint32_t> rng(2 * (size_t)nn), refs(2 * (size_t)nn), level_count;
  rng[0] = 0, rng[1] = n;
  uint32_t begin = 0, count = 1, depth = 0;
  while (count) {
    uint32_t next = begin + count;
    for (uint32_t x = begin; x < begin + count; ++x) {
      const uint32_t lo = rng[2 * x], hi = rng[2 * x + 1];
      assert(hi - lo >= 2 && depth + rtwb::need_of(hi - lo) <= cap);  // hence depth <= cap
      const uint32_t m = rtwb::split_of(keys.data(), lo, hi, depth, cap);
      assert(lo < m && m < hi);
      const uint32_t cb[2] = {lo, m}, ce[2] = {m, hi};
      for (int c = 0; c < 2; ++c) {
        if (ce[c] - cb[c] > 1u) {
          assert(next < nn);
          rng[2 * next] = cb[c], rng[2 * next + 1] = ce[c];
          refs[2 * x + c] = next++;
        } else {
          refs[2 * x + c] = rtwb::leaf_ref(cb[c]);
        }
      }
    }
    level_count.push_back(count);
    begin += count, count = next - begin, ++depth;
  }
  assert(begin == nn && depth <= cap && depth <= rtwb::kMaxLevels);

  // permute: the order table, each record's meta doubles (11, 14-15) at its new position
  std::vector<double> meta(3 * (size_t)n);
  for (uint32_t pos = 0; pos < n; ++pos) {
    const double* s = prim + (size_t)rtwk::kWorldRec * order[sorted[pos]];
    meta[3 * (size_t)pos] = s[11], meta[3 * (size_t)pos + 1] = s[14], meta[3 * (size_t)pos + 2] = s[15];
  }
  std::vector<uint32_t> elig(n);  // per new position: a leaf the pretest may hold (judged on the new numbers)
  for (uint32_t pos = 0; pos < n; ++pos) {
    double* d = prim + (size_t)rtwk::kWorldRec * pos;
    d[11] = meta[3 * (size_t)pos], d[14] = meta[3 * (size_t)pos + 1], d[15] = meta[3 * (size_t)pos + 2];
    const uint32_t li = sorted[pos];
    order[li] = pos;
    elig[pos] = rtwr::eligible(rtwr::ld_u32(d + 14, 0), a + (size_t)9 * li) ? 1u : 0u;
    mate[li] = elig[pos] ? li : rtwr::kNone;
    if (k.has_cull && !elig[pos]) std::memset(cull + (size_t)16 * pos, 0, 16 * sizeof(float));
  }
  // refit tables: refs, candidates, the schedule (levels, the deepest first)
  std::vector<uint32_t> level_off(depth + 1, 0u);
  for (uint32_t l = 0; l < depth; ++l) level_off[l + 1] = level_off[l] + level_count[l];
  for (uint32_t l = 0; l < depth; ++l)
    for (uint32_t x = level_off[l]; x < level_off[l + 1]; ++x) {
      uint32_t cd = 0;
      for (int c = 0; c < 2; ++c) {
        const uint32_t ref = refs[2 * x + c];
        rtwr::st_u32(node + (size_t)rtwk::kNodeWords * x, 12 + c, ref);
        if ((ref & rtwk::kLeafBit) && elig[ref & 0x7FFFFFu]) cd |= 1u << c;
      }
      cand[x] = cd;
      const uint32_t at = rtwb::sched_place(nn, level_off[l], level_off[l + 1], x);
      by_height[at] = x, heights[at] = rtwb::sched_label(depth, l);
    }
  level_schedule(level_count.data(), depth, nn, r);
  k.info[2] = depth;
  return RTW_OK;
}

}  // namespace rtwp
