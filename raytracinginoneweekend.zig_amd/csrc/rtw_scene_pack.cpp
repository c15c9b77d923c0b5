// rtw_scene_pack.cpp — builds the cover scene's device tables
// (rtw_scene_pack.hpp; layout: rtw_internal.hpp).  Plain C++: no HIP, no
// environment.
#include "rtw_scene_pack.hpp"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "rtw_cull.hpp"
#include "rtw_layout.hpp"

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

// bit 16 of a pair's time-group word: both spheres of the pair move along y
// only (ndc.x == ndc.z == 0): the kernel's pretest then skips the x and z
// centre updates.
void flag_y_only(const std::vector<float>& recs, std::vector<uint32_t>& tg, uint32_t pairs) {
  for (uint32_t p = 0; p < pairs; ++p) {
    const float* q = &recs[(size_t)16 * p];
    if (q[6] == 0.0f && q[7] == 0.0f && q[10] == 0.0f && q[11] == 0.0f) tg[p] |= 1u << 16;
  }
}

}  // namespace

int pack_scene(const rtw_sphere* spheres, uint32_t n, const rtw_material* mats, uint32_t nm, ScenePack& out,
               std::string& msg) {
  if (n > 0 && !spheres) return fail(msg, RTW_EINVAL, "rtw_scene_create: spheres is NULL");
  if (nm > 0 && !mats) return fail(msg, RTW_EINVAL, "rtw_scene_create: materials is NULL");
  if (n > RTW_MAX_SPHERES || nm > RTW_MAX_SPHERES)
    return fail(msg, RTW_UNSUPPORTED, "rtw_scene_create: %u spheres / %u materials exceeds %u (BVH path not built)",
                n, nm, RTW_MAX_SPHERES);
  for (uint32_t i = 0; i < nm; ++i) {
    if (mats[i].kind > RTW_DIELECTRIC)
      return fail(msg, RTW_UNSUPPORTED, "material %u: kind %u not supported on the GPU path", i, mats[i].kind);
  }
  // Distinct (t0, t1) pairs of moving spheres -> time groups.
  std::vector<std::pair<double, double>> groups;
  std::vector<uint32_t> meta_orig(n, 0u);
  uint32_t n_moving = 0, n_wide = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const rtw_sphere& s = spheres[i];
    if (s.mat >= nm) return fail(msg, RTW_EINVAL, "sphere %u: material index %u >= %u", i, s.mat, nm);
    if (s.moving > 1) return fail(msg, RTW_EINVAL, "sphere %u: moving flag %u", i, s.moving);
    uint32_t m = (s.mat << 8) | (i << 20);
    if (s.moving) {
      ++n_moving;
      uint32_t g = 0;
      while (g < groups.size() && !(groups[g].first == s.t0 && groups[g].second == s.t1)) ++g;
      if (g == groups.size()) {
        if (groups.size() >= rtwk::kMaxTimeGroups)
          return fail(msg, RTW_UNSUPPORTED, "more than %u distinct moving-sphere time ranges", rtwk::kMaxTimeGroups);
        groups.emplace_back(s.t0, s.t1);
      }
      m |= rtwk::kMoving | (g << 2);
    }
    if (s.radius >= rtwk::kWideRadius) {
      m |= rtwk::kWide;
      ++n_wide;
    }
    meta_orig[i] = m;
  }
  // Table order [static wide | static | moving wide | moving], list order within
  // each group (rtw_internal.hpp); perm[i] = table position of sphere i.
  std::vector<uint32_t> order;
  order.reserve(n);
  for (int grp = 0; grp < 4; ++grp)
    for (uint32_t i = 0; i < n; ++i) {
      const bool mv = (meta_orig[i] & rtwk::kMoving) != 0, wd = (meta_orig[i] & rtwk::kWide) != 0;
      if ((int)mv * 2 + (int)!wd == grp) order.push_back(i);
    }
  uint32_t g_end[4] = {0, 0, 0, 0};
  for (uint32_t i = 0; i < n; ++i) {
    const bool mv = (meta_orig[i] & rtwk::kMoving) != 0, wd = (meta_orig[i] & rtwk::kWide) != 0;
    for (int grp = (int)mv * 2 + (int)!wd; grp < 4; ++grp) ++g_end[grp];
  }
  std::vector<uint32_t> meta(n + 1, 0u), perm(n, 0u);
  for (uint32_t k = 0; k < n; ++k) {
    meta[k] = meta_orig[order[k]];
    perm[order[k]] = k;
  }
  const uint32_t ng = (uint32_t)groups.size();
  // Host tables (rtw_internal.hpp has the layout).  Reciprocals are correctly
  // rounded IEEE divisions: the kernel's div_rn needs y = RN(1/b).
  // sph / meta carry one zero padding record: the sphere loop prefetches k+1.
  std::vector<double> sph64((size_t)8 * (n + 1), 0.0), rad64(n), mat64((size_t)8 * nm), tg64((size_t)4 * ng);
  std::vector<float> sph32((size_t)8 * (n + 1), 0.0f), rad32(n), mat32((size_t)8 * nm), tg32((size_t)4 * ng);
  std::vector<uint32_t> kind(nm);
  for (uint32_t i = 0; i < n; ++i) {  // i = table position
    const rtw_sphere& s = spheres[order[i]];
    const double rec[8] = {s.c0[0], s.c0[1], s.c0[2], s.c1[0] - s.c0[0], s.c1[1] - s.c0[1], s.c1[2] - s.c0[2],
                           s.radius * s.radius, 1.0 / s.radius};
    for (int k = 0; k < 8; ++k) sph64[8 * i + k] = rec[k];
    for (int k = 0; k < 6; ++k) sph32[8 * i + k] = (float)rec[k];
    const float rf = (float)s.radius;
    sph32[8 * i + 6] = rf * rf;  // f32 mode: r*r in f32 (tierb_core.h prep)
    sph32[8 * i + 7] = 1.0f / rf;
    rad64[i] = s.radius;
    rad32[i] = rf;
  }
  for (uint32_t i = 0; i < nm; ++i) {
    const rtw_material& m = mats[i];
    const bool diel = m.kind == RTW_DIELECTRIC;
    const double rec[8] = {m.albedo[0], m.albedo[1], m.albedo[2], m.albedo_odd[0], m.albedo_odd[1],
                           m.albedo_odd[2], diel ? 1.0 / m.ir : m.fuzz, m.ir};
    for (int k = 0; k < 8; ++k) {
      mat64[8 * i + k] = rec[k];
      mat32[8 * i + k] = (float)rec[k];
    }
    if (diel) {
      mat32[8 * i + 6] = 1.0f / (float)m.ir;
      // Schlick's r0^2 (material.zig:87-91) for ratio = RN(1/ir) (front face)
      // and ir (back face), with the kernel's operations in each precision.
      for (int f = 0; f < 2; ++f) {
        const double rd = f == 0 ? mat64[8 * i + 6] : m.ir;
        const double r0d = (1.0 - rd) / (1.0 + rd);
        mat64[8 * i + f] = r0d * r0d;
        const float rf = f == 0 ? mat32[8 * i + 6] : (float)m.ir;
        const float r0f = (1.0f - rf) / (1.0f + rf);
        mat32[8 * i + f] = r0f * r0f;
      }
    }
    kind[i] = m.kind;
  }
  for (uint32_t g = 0; g < ng; ++g) {
    const double t0 = groups[g].first, t1 = groups[g].second;
    tg64[4 * g] = t0;
    tg64[4 * g + 1] = t1;
    tg64[4 * g + 2] = 1.0 / (t1 - t0);
    const float f0 = (float)t0, f1 = (float)t1;
    tg32[4 * g] = f0;
    tg32[4 * g + 1] = f1;
    tg32[4 * g + 2] = 1.0f / (f1 - f0);
  }
  // Pretest records (rtw_cull.hpp) over the narrow spheres in table order:
  // narrow index j -> table position (static narrow first, then moving narrow).
  const uint32_t n_sn = g_end[1] - g_end[0], nn = n_sn + (n - g_end[2]);
  const uint32_t nn_pad = (nn + 31u) & ~31u;
  auto table_pos = [&](uint32_t j) { return j < n_sn ? g_end[0] + j : g_end[2] + (j - n_sn); };
  auto group_of = [&](uint32_t pos) { return (meta[pos] & rtwk::kMoving) ? (meta[pos] >> 2) & 63u : 0u; };
  std::vector<float> cull((size_t)8 * nn_pad + 16, 0.0f);  // + one padding pair (prefetch)
  std::vector<uint32_t> cull_tg(nn_pad / 2 + 1, 0u);
  double cmax_c = 0.0, cmax_d = 0.0, rho_max = 1.0;
  for (uint32_t j = 0; j < nn; ++j) {
    const uint32_t pos = table_pos(j);
    const double* r = &sph64[8 * pos];
    float* q = &cull[(size_t)16 * (j / 2) + (j & 1)];
    for (int k = 0; k < 3; ++k) {
      q[2 * k] = (float)r[k];
      q[2 * (3 + k)] = -(float)r[3 + k];
      cmax_c = std::max(cmax_c, std::fabs(r[k]));
      cmax_d = std::max(cmax_d, std::fabs(r[3 + k]));
    }
    const float rf = (float)rad64[pos];
    q[12] = -(rf * rf);
    rho_max = std::max(rho_max, 2.0 * r[6] + 1.0);
    cull_tg[j / 2] |= group_of(pos) << (8 * (j & 1));
  }
  for (uint32_t j = nn; j < nn_pad; ++j)  // padding: same time group as its partner
    if (j & 1) cull_tg[j / 2] |= (cull_tg[j / 2] & 0xFFu) << 8;
  for (uint32_t j = 0; j + 1 < nn; j += 2) {  // static half of a mixed pair: partner's group
    const bool m0 = j >= n_sn, m1 = j + 1 >= n_sn;
    if (!m0 && m1) cull_tg[j / 2] = (cull_tg[j / 2] & 0xFF00u) | (cull_tg[j / 2] >> 8);
  }
  flag_y_only(cull, cull_tg, nn_pad / 2);
  const float cmax = std::nextafter((float)(cmax_c + cmax_d), INFINITY);
  const float rho = std::nextafter((float)rho_max, INFINITY);
  const uint32_t cull_on = (nn > 0 && cmax <= rtwc::kCmaxLimit) ? 1u : 0u;
  // Clustered pretest tables (SceneView ccull...; rtw_device.hpp closest_hit, f64).
  // kd-split of the narrow spheres (by the centre of their swept box over
  // the shutter) into clusters of <= 8; members static first, so pairs are
  // static-static where possible.  Bounding sphere of cluster c: centre
  // C = f32(centre of the members' swept box), radius R = max over members
  // of max(|c0 - C|, |c1 - C|) + |r|, widened by 1e-4 (1 + R): a line whose
  // f64 discriminant for (C, R) is negative passes every member at a distance
  // above its radius + 1e-4, far beyond the f64 rounding of the member's own
  // exact test, which therefore rejects it.  Valid for
  // sphere times within each time group's [t0, t1] (checked per render).
  std::vector<uint32_t> cl_items;  // j (narrow index) per slot, ~0u = dummy
  std::vector<float> cclus;
  double cmax_cl = 0.0, rho_cl = 1.0;
  {
    auto cen_of = [&](uint32_t j, int k) {
      const double* r = &sph64[8 * table_pos(j)];
      return r[k] + 0.5 * r[3 + k];
    };
    std::vector<std::vector<uint32_t>> parts;
    std::vector<uint32_t> all(nn);
    for (uint32_t j = 0; j < nn; ++j) all[j] = j;
    if (nn) parts.push_back(all);
    for (bool again = true; again;) {
      again = false;
      for (size_t gi = 0; gi < parts.size(); ++gi) {
        if (parts[gi].size() <= rtwk::kClusterSlots) continue;
        std::vector<uint32_t> g = parts[gi];
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t j : g)
          for (int k = 0; k < 3; ++k) lo[k] = std::min(lo[k], cen_of(j, k)), hi[k] = std::max(hi[k], cen_of(j, k));
        int ax = 0;
        for (int k = 1; k < 3; ++k)
          if (hi[k] - lo[k] > hi[ax] - lo[ax]) ax = k;
        std::stable_sort(g.begin(), g.end(), [&](uint32_t a, uint32_t b) { return cen_of(a, ax) < cen_of(b, ax); });
        // Split sizes: whole clusters of 8 on the left, ceil(n/8) clusters in
        // all (profiles/r02/cluster_ab.txt: fewer, fuller clusters beat
        // smaller ones whose bounds are tighter: each cluster costs a ballot
        // and a branch per wave-iteration).
        constexpr size_t CS = rtwk::kClusterSlots;
        const size_t h = CS * (((g.size() + CS - 1) / CS) / 2);
        parts[gi].assign(g.begin(), g.begin() + h);
        parts.emplace_back(g.begin() + h, g.end());
        again = true;
      }
    }
    for (auto& g : parts) {
      std::stable_sort(g.begin(), g.end(), [&](uint32_t a, uint32_t b) { return (a >= n_sn) < (b >= n_sn); });
      double mc0[rtwk::kClusterSlots][3], mdc[rtwk::kClusterSlots][3], mr[rtwk::kClusterSlots];
      for (size_t i = 0; i < g.size(); ++i) {
        const uint32_t pos = table_pos(g[i]);
        for (int k = 0; k < 3; ++k) mc0[i][k] = sph64[8 * pos + k], mdc[i][k] = sph64[8 * pos + 3 + k];
        mr[i] = rad64[pos];
      }
      float cf[3], rf;
      rtwc::cluster_sphere(mc0, mdc, mr, (int)g.size(), cf, rf);
      const size_t c = cl_items.size() / rtwk::kClusterSlots;
      if (cclus.size() < 16 * (c / 2 + 1)) cclus.resize(16 * (c / 2 + 1), 0.0f);
      float* q = &cclus[16 * (c / 2) + (c & 1)];
      for (int k = 0; k < 3; ++k) q[2 * k] = cf[k], cmax_cl = std::max(cmax_cl, (double)std::fabs(cf[k]));
      q[12] = -(rf * rf);
      rho_cl = std::max(rho_cl, 2.0 * (double)rf * (double)rf + 1.0);
      for (uint32_t i = 0; i < rtwk::kClusterSlots; ++i) cl_items.push_back(i < g.size() ? g[i] : ~0u);
    }
  }
  const uint32_t n_clusters = (uint32_t)(cl_items.size() / rtwk::kClusterSlots);
  const uint32_t n_cslots = rtwk::kClusterSlots * n_clusters;
  // slot tables; a dummy slot's record (c = 0, nr2 = +3e38) is a proven miss for every lane
  std::vector<float> ccull((size_t)8 * n_cslots + 16, 0.0f);
  std::vector<uint32_t> ccull_tg(n_cslots / 2 + 1, 0u), cpos(std::max(n_cslots, 1u), 0u);
  std::vector<uint32_t> cvalid(2 * ((n_cslots + 63) / 64) + 2, 0u);
  for (uint32_t sl = 0; sl < n_cslots; ++sl) {
    float* q = &ccull[(size_t)16 * (sl / 2) + (sl & 1)];
    const uint32_t j = cl_items[sl];
    if (j == ~0u) {
      q[12] = 3e38f;
      continue;
    }
    const float* src = &cull[(size_t)16 * (j / 2) + (j & 1)];  // the member's own pretest record
    for (int k = 0; k < 7; ++k) q[2 * k] = src[2 * k];
    cpos[sl] = table_pos(j);
    cvalid[2 * (sl / 64) + ((sl % 64) >> 5)] |= 0x80000000u >> (sl & 31u);
    ccull_tg[sl / 2] |= group_of(cpos[sl]) << (8 * (sl & 1));
  }
  for (uint32_t p = 0; p < n_cslots / 2; ++p) {
    const uint32_t j0 = cl_items[2 * p], j1 = cl_items[2 * p + 1];
    const bool m0 = j0 != ~0u && j0 >= n_sn, m1 = j1 != ~0u && j1 >= n_sn;
    if (!m0 && !m1) ccull_tg[p] |= 1u << 17;  // static pair (dummies count as static)
    if (!m0 && m1) ccull_tg[p] = (ccull_tg[p] & 0xFF00u) | ((ccull_tg[p] >> 8) & 0xFFu) | (ccull_tg[p] & ~0xFFFFu);
    if (m0 && !m1) ccull_tg[p] = (ccull_tg[p] & 0xFFu) | ((ccull_tg[p] & 0xFFu) << 8) | (ccull_tg[p] & ~0xFFFFu);
  }
  flag_y_only(ccull, ccull_tg, n_cslots / 2);
  if (cclus.empty()) cclus.assign(16, 0.0f);
  const float cmax_all = std::max(cmax, std::nextafter((float)cmax_cl, INFINITY));
  const float rho_c = std::nextafter((float)rho_cl, INFINITY);
  // One blob: each table at a 256-B aligned offset, 8 spare bytes after each.
  out = ScenePack{};
  auto put = [&](SceneTable t, const auto& v) {
    const size_t bytes = v.size() * sizeof(v[0]);
    out.off[t] = out.blob.size();
    out.blob.resize(out.blob.size() + ((bytes + 8 + 255) & ~(size_t)255), 0);
    if (bytes) std::memcpy(out.blob.data() + out.off[t], v.data(), bytes);
  };
  put(kSph64, sph64), put(kRad64, rad64), put(kMat64, mat64), put(kTg64, tg64);
  put(kSph32, sph32), put(kRad32, rad32), put(kMat32, mat32), put(kTg32, tg32);
  put(kMeta, meta), put(kKind, kind), put(kPerm, perm);
  put(kCull, cull), put(kCullTg, cull_tg);
  put(kCcull, ccull), put(kCcullTg, ccull_tg), put(kCclus, cclus), put(kCpos, cpos), put(kCvalid, cvalid);
  out.n = n, out.nm = nm, out.ng = ng;
  for (int k = 0; k < 3; ++k) out.g_end[k] = g_end[k];
  out.nn = nn, out.nn_pad = nn_pad, out.n_sn = n_sn;
  out.cull_on = cull_on, out.cmax = cmax, out.rho = rho;
  out.n_clusters = n_clusters;
  out.cluster_ok = (n_clusters > 0 && cull_on && cmax_all <= rtwc::kCmaxLimit) ? 1u : 0u;
  out.cmax_all = cmax_all, out.rho_c = rho_c;
  out.n_static = n - n_moving, out.n_moving = n_moving, out.n_wide = n_wide;
  out.groups = std::move(groups);
  return RTW_OK;
}

}  // namespace rtwp
