// rtw_world_refit.cpp — the host side of a dynamic world (rtw_hip.h
// RTW_WORLD_DYNAMIC): the refit tables made at creation, and the host refit
// that defines what an update leaves in the device tables
// (rtw_world_update.hip runs the same per-item steps, rtw_world_refit.hpp).
// Plain C++: no HIP, no environment.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>

#include "rtw_cull.hpp"
#include "rtw_layout.hpp"
#include "rtw_world_pack.hpp"
#include "rtw_tri.hpp"
#include "rtw_world_refit.hpp"

namespace rtwp {

rtwr::View refit_view(WorldPack& k, RefitPack& r, const double* a, const double* xv) {
  rtwr::View V{};
  unsigned char* b = k.blob.data();
  unsigned char* rb = r.blob.data();
  V.prim = reinterpret_cast<double*>(b + k.o_prim);
  V.xform = reinterpret_cast<double*>(b + k.o_xform);
  V.node = reinterpret_cast<float*>(b + k.o_node);
  V.order = reinterpret_cast<const uint32_t*>(b + k.o_order);
  V.cull = reinterpret_cast<float*>(b + k.o_cull);
  V.by_height = reinterpret_cast<const uint32_t*>(rb + r.o_by_height);
  V.heights = reinterpret_cast<const uint32_t*>(rb + r.o_heights);
  V.plain = reinterpret_cast<float*>(rb + r.o_plain);
  V.cand = reinterpret_cast<const uint32_t*>(rb + r.o_cand);
  V.mate = reinterpret_cast<const uint32_t*>(rb + r.o_mate);
  V.a = a, V.xv = xv;
  V.n_prims = k.n_prims, V.n_xforms = r.n_xforms, V.n_nodes = k.n_nodes;
  V.packed = k.packed ? 1u : 0u, V.has_table = k.has_cull ? 1u : 0u, V.cull_on = 0u;
  V.has_tri = (k.feat & 64u) ? 1u : 0u;
  return V;
}

void make_refit(const rtw_world_desc* d, const WorldPack& k, RefitPack& out) {
  RefitPack r;
  const uint32_t n = k.n_prims, nn = k.n_nodes;
  r.n_xforms = d->n_xforms;
  for (uint32_t i = 0; i < n; ++i)
    r.kind.push_back(d->prims[i].kind), r.mat.push_back(d->prims[i].mat), r.xform.push_back(d->prims[i].xform);
  for (uint32_t i = 0; i < d->n_xforms; ++i) {
    uint32_t h = d->xforms[i].n;
    for (uint32_t c = 0; c < d->xforms[i].n; ++c) h |= d->xforms[i].op[c] << (8 + 4 * c);
    r.xf_header.push_back(h);
  }
  const float* nodes = reinterpret_cast<const float*>(k.blob.data() + k.o_node);
  const uint32_t* order = reinterpret_cast<const uint32_t*>(k.blob.data() + k.o_order);
  std::vector<uint32_t> list_of(n);  // stored position -> list index
  for (uint32_t li = 0; li < n; ++li) list_of[order[li]] = li;
  auto ref_of = [&](uint32_t nd, int c) { return rtwr::ld_u32(nodes + (size_t)rtwk::kNodeWords * nd, 12 + c); };

  // heights (1: both children are leaves), nodes sorted by them
  std::vector<uint32_t> height(nn, 0u);
  std::function<uint32_t(uint32_t)> walk = [&](uint32_t nd) {
    uint32_t h = 0;
    for (int c = 0; c < 2; ++c) {
      const uint32_t ref = ref_of(nd, c);
      if (!(ref & rtwk::kLeafBit)) h = std::max(h, walk(ref));
    }
    return height[nd] = h + 1;
  };
  if (nn) r.h_max = walk(0);
  std::vector<uint32_t> by_height(nn), heights(nn);
  for (uint32_t i = 0; i < nn; ++i) by_height[i] = i;
  std::stable_sort(by_height.begin(), by_height.end(), [&](uint32_t x, uint32_t y) { return height[x] < height[y]; });
  r.h_off.assign(r.h_max + 1, 0u);
  for (uint32_t i = 0; i < nn; ++i) heights[i] = height[by_height[i]], r.h_off[heights[i]]++;
  for (uint32_t h = 1; h <= r.h_max; ++h) r.h_off[h] += r.h_off[h - 1];
  r.h_star = 1;
  while (r.h_star < r.h_max && nn - r.h_off[r.h_star - 1] > rtwr::kBlock) ++r.h_star;

  // the bounds before pack_refs: a leaf child's from its primitives, an
  // interior child's as the union of that child's own two (what pack_world's
  // range_box rounds to: outward rounding is monotone)
  std::vector<float> plain((size_t)12 * nn, 0.0f);
  std::vector<uint32_t> cand(nn, 0u), mate(n, rtwr::kNone);
  for (uint32_t i = 0; i < nn; ++i) {
    const uint32_t nd = by_height[i];
    for (int c = 0; c < 2; ++c) {
      const uint32_t ref = ref_of(nd, c);
      float* pl = plain.data() + (size_t)12 * nd;
      if (ref & rtwk::kLeafBit) {
        const uint32_t first = ref & 0x7FFFFFu, cnt = (ref >> 23) & rtwk::kLeafCountMask;
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        bool ok = cnt >= 1 && cnt <= 2;
        for (uint32_t pos = first; pos < first + cnt; ++pos) {
          const rtw_prim& p = d->prims[list_of[pos]];
          const uint32_t meta0 = p.kind | ((uint32_t)(p.xform + 1) << 8);
          double bl[3], bh[3];
          rtwr::prim_box(p.kind, p.a, p.xform >= 0 ? r.xf_header[p.xform] : 0u,
                         p.xform >= 0 ? &d->xforms[p.xform].v[0][0] : p.a, bl, bh);
          for (int a = 0; a < 3; ++a) lo[a] = rtwr::dmin(lo[a], bl[a]), hi[a] = rtwr::dmax(hi[a], bh[a]);
          ok = ok && rtwr::eligible(meta0, p.a);
        }
        for (int a = 0; a < 3; ++a) pl[2 * a + c] = rtwr::down(lo[a]), pl[6 + 2 * a + c] = rtwr::up(hi[a]);
        if (ok) {
          cand[nd] |= 1u << c;
          for (uint32_t j = 0; j < cnt; ++j) mate[list_of[first + j]] = list_of[first + (cnt - 1 - j)];
        }
      } else {
        const float* q = plain.data() + (size_t)12 * ref;
        for (int a = 0; a < 3; ++a)
          pl[2 * a + c] = rtwr::fmin32(q[2 * a], q[2 * a + 1]), pl[6 + 2 * a + c] = rtwr::fmax32(q[6 + 2 * a], q[7 + 2 * a]);
      }
    }
  }
  auto put = [&](size_t& o, const auto& v) {
    const size_t bytes = v.size() * sizeof(v[0]);
    o = r.blob.size();
    r.blob.resize(o + ((std::max(bytes, (size_t)4) + 255) & ~(size_t)255), 0);
    if (bytes) std::memcpy(r.blob.data() + o, v.data(), bytes);
  };
  put(r.o_by_height, by_height), put(r.o_heights, heights), put(r.o_plain, plain), put(r.o_cand, cand), put(r.o_mate, mate);
  out = std::move(r);
}

bool same_fixed_fields(const RefitPack& r, const rtw_prim* prims, uint32_t n_prims, const rtw_xform* xforms,
                       uint32_t n_xforms, std::string& msg) {
  char buf[160];
  if (n_prims != r.kind.size() || n_xforms != r.n_xforms) {
    snprintf(buf, sizeof(buf), "%u primitives / %u transforms, the world has %zu / %u", n_prims, n_xforms, r.kind.size(),
             r.n_xforms);
    msg = buf;
    return false;
  }
  for (uint32_t i = 0; i < n_prims; ++i)
    if (prims[i].kind != r.kind[i] || prims[i].mat != r.mat[i] || prims[i].xform != r.xform[i]) {
      snprintf(buf, sizeof(buf), "prim %u: kind / material / xform differ from the world's", i);
      msg = buf;
      return false;
    }
  for (uint32_t i = 0; i < n_xforms; ++i) {
    uint32_t h = xforms[i].n;
    for (uint32_t c = 0; c < xforms[i].n && c < RTW_MAX_XFORM_OPS; ++c) h |= (xforms[i].op[c] & 0xFu) << (8 + 4 * c);
    if (xforms[i].n > RTW_MAX_XFORM_OPS || h != r.xf_header[i]) {
      snprintf(buf, sizeof(buf), "xform %u: its ops differ from the world's", i);
      msg = buf;
      return false;
    }
  }
  return true;
}

int refit_world(WorldPack& k, RefitPack& r, const double* a, const double* xv) {
  rtwr::View V = refit_view(k, r, a, xv);
  rtwr::Partial p;
  rtwr::partial_init(p);
  for (uint32_t i = 0; i < V.n_prims; ++i) rtwr::validate_prim(V, i, p);
  for (uint32_t i = 0; i < V.n_xforms; ++i) rtwr::validate_xform(V, i, p);
  if (p.bad != 0.0) {
    r.msg = refit_violation(p.bad, p.first_bad, V.n_prims);
    return RTW_EINVAL;
  }
  refit_scalars(p, V.n_nodes, k.cull_cmax, k.cull_rho, k.bounds_lo, k.bounds_hi);
  V.cull_on = V.has_table && k.cull_cmax <= rtwc::kCmaxLimit;
  for (uint32_t i = 0; i < V.n_prims; ++i) rtwr::commit_prim(V, i);
  for (uint32_t i = 0; i < V.n_xforms; ++i) rtwr::commit_xform(V, i);
  for (uint32_t i = 0; i < V.n_nodes; ++i) rtwr::commit_node(V, V.by_height[i]);
  return RTW_OK;
}

std::string refit_violation(double bad, double first_bad, uint32_t n_prims) {
  char buf[200];
  if (first_bad < (double)n_prims)
    snprintf(buf, sizeof(buf), "update: %.0f violations, the first at prim %.0f (a used number is not finite, or a moving sphere's time1 <= time0)",
             bad, first_bad);
  else
    snprintf(buf, sizeof(buf), "update: %.0f violations, the first at xform %.0f (a value is not finite)", bad,
             first_bad - (double)n_prims);
  return buf;
}

void refit_scalars(const rtwr::Partial& p, uint32_t n_nodes, float& cull_cmax, float& cull_rho, double lo[3], double hi[3]) {
  for (int c = 0; c < 3; ++c) lo[c] = p.lo[c], hi[c] = p.hi[c];
  if (!n_nodes) return;  // (a world without a BVH has no pretest: both stay 0)
  cull_cmax = rtwr::next_up((float)(p.cc + p.cd));
  cull_rho = rtwr::next_up((float)p.rho);
}

}  // namespace rtwp
