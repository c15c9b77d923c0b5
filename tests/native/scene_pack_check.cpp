// The cover scene's device tables (csrc/rtw_scene_pack.cpp, layout in
// csrc/rtw_internal.hpp) against the spheres and materials they were made
// from: table order and permutation, the f64 / f32 records, the pretest pair
// records with their time-group bytes and flags, the clusters' slot tables and
// bounding spheres, and the bounds cmax / rho.  The expectations are restated
// here from the layout's description, not taken from the packer.
//
// Inputs: the cover scene at seed 42; a generated scene of 101 narrow spheres
// in three time groups (static, movers along x, along y only and along z) with
// a static and a moving sphere of radius >= 100; and the edges n = 0, n = 1,
// movers only, an odd narrow count, kClusterSlots + 1 narrow spheres.
//
// usage: scene_pack_check [DUMP_DIR]  ->  "scenes S checks C violations V",
// exit 1 if V > 0.  With DUMP_DIR the blobs of the first two scenes are
// written there (cover42.blob, gen101.blob) for the digest comparison.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pack_inputs.hpp"
#include "rtw_cull.hpp"
#include "rtw_layout.hpp"
#include "rtw_scene_pack.hpp"

namespace {

long g_checks = 0, g_viol = 0;
const char* g_scene = "";
#define CHECK(cond, ...)                               \
  do {                                                 \
    ++g_checks;                                        \
    if (!(cond) && g_viol++ < 20) {                    \
      fprintf(stderr, "%s: %s: ", g_scene, #cond);     \
      fprintf(stderr, __VA_ARGS__);                    \
      fprintf(stderr, "\n");                           \
    }                                                  \
  } while (0)

template <typename T>
bool same_bits(T a, T b) {
  return std::memcmp(&a, &b, sizeof(T)) == 0;
}

// The time-group word of a pair of slots.  A slot is absent (padding / dummy),
// static, or moving in group g.  Byte of a moving slot: its group; of a static
// slot beside a moving one: the partner's; of an absent slot: its partner's
// byte; else 0.  bit 16: neither slot moves along x or z; bit 17 (cluster
// table only): no moving slot.
struct Slot {
  bool real = false, moving = false;
  uint32_t group = 0;
  float ndc_x = 0.0f, ndc_z = 0.0f;
};
uint32_t expected_tg(const Slot& a, const Slot& b, bool static_bit) {
  auto byte = [](const Slot& s, const Slot& o) { return s.real && s.moving ? s.group : (o.real && o.moving ? o.group : 0u); };
  uint32_t w = byte(a, b) | (byte(b, a) << 8);
  if (a.ndc_x == 0.0f && a.ndc_z == 0.0f && b.ndc_x == 0.0f && b.ndc_z == 0.0f) w |= 1u << 16;
  if (static_bit && !(a.real && a.moving) && !(b.real && b.moving)) w |= 1u << 17;
  return w;
}

void verify(const char* name, const std::vector<rtw_sphere>& sph, const std::vector<rtw_material>& mats,
            const rtwp::ScenePack& k) {
  g_scene = name;
  const uint32_t n = (uint32_t)sph.size(), nm = (uint32_t)mats.size();
  constexpr uint32_t CS = rtwk::kClusterSlots;
  auto D = [&](rtwp::SceneTable t) { return reinterpret_cast<const double*>(k.blob.data() + k.off[t]); };
  auto F = [&](rtwp::SceneTable t) { return reinterpret_cast<const float*>(k.blob.data() + k.off[t]); };
  auto U = [&](rtwp::SceneTable t) { return reinterpret_cast<const uint32_t*>(k.blob.data() + k.off[t]); };
  const long viol_before = g_viol;
  for (int t = 0; t < rtwp::kSceneTables; ++t) {
    CHECK(k.off[t] % 256 == 0 && k.off[t] < k.blob.size(), "table %d at %zu of %zu", t, k.off[t], k.blob.size());
    if (t) CHECK(k.off[t] > k.off[t - 1], "table %d not after table %d", t, t - 1);
  }
  if (g_viol != viol_before) return;  // (the reads below rely on the offsets)
  CHECK(k.n == n && k.nm == nm, "n %u nm %u", k.n, k.nm);

  // ---- groups, order, perm, meta
  std::vector<std::pair<double, double>> groups;
  std::vector<uint32_t> grp(n), tgroup(n, 0u);
  uint32_t count[4] = {0, 0, 0, 0}, n_moving = 0, n_wide = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const bool wide = sph[i].radius >= 100.0, mv = sph[i].moving != 0;
    grp[i] = (mv ? 2u : 0u) + (wide ? 0u : 1u);  // static wide, static, moving wide, moving
    ++count[grp[i]];
    n_moving += mv, n_wide += wide;
    if (mv) {
      uint32_t g = 0;
      while (g < groups.size() && !(groups[g].first == sph[i].t0 && groups[g].second == sph[i].t1)) ++g;
      if (g == groups.size()) groups.emplace_back(sph[i].t0, sph[i].t1);
      tgroup[i] = g;
    }
  }
  const uint32_t end[4] = {count[0], count[0] + count[1], count[0] + count[1] + count[2], n};
  CHECK(k.g_end[0] == end[0] && k.g_end[1] == end[1] && k.g_end[2] == end[2], "group ends %u %u %u, expected %u %u %u",
        k.g_end[0], k.g_end[1], k.g_end[2], end[0], end[1], end[2]);
  CHECK(k.n_moving == n_moving && k.n_static == n - n_moving && k.n_wide == n_wide, "counts %u %u %u", k.n_static,
        k.n_moving, k.n_wide);
  CHECK(k.ng == groups.size() && k.groups == groups, "time groups %u, expected %zu", k.ng, groups.size());
  const uint32_t *perm = U(rtwp::kPerm), *meta = U(rtwp::kMeta);
  std::vector<uint32_t> list_of(n, ~0u);  // table position -> list index
  uint32_t next[4] = {0, end[0], end[1], end[2]};
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t want = next[grp[i]]++;  // list order inside each group
    CHECK(perm[i] == want, "perm[%u] = %u, expected %u", i, perm[i], want);
    if (perm[i] >= n || list_of[perm[i]] != ~0u) {
      CHECK(false, "perm is no permutation at %u", i);
      return;
    }
    list_of[perm[i]] = i;
    const uint32_t m = meta[perm[i]];
    CHECK(m >> 20 == i, "meta[perm[%u]] >> 20 = %u", i, m >> 20);
    CHECK(((m & rtwk::kMoving) != 0) == (sph[i].moving != 0) && ((m & rtwk::kWide) != 0) == (sph[i].radius >= 100.0),
          "meta flags of sphere %u: %x", i, m);
    CHECK(((m >> 8) & 0xFFFu) == sph[i].mat, "meta material of sphere %u", i);
    CHECK(((m >> 2) & 63u) == tgroup[i], "meta time group of sphere %u: %u, expected %u", i, (m >> 2) & 63u, tgroup[i]);
  }
  CHECK(meta[n] == 0u, "meta padding record %x", meta[n]);

  // ---- sphere, radius, material and time-group tables, f64 and the documented f32 roundings
  const double *s64 = D(rtwp::kSph64), *r64 = D(rtwp::kRad64), *m64 = D(rtwp::kMat64), *t64 = D(rtwp::kTg64);
  const float *s32 = F(rtwp::kSph32), *r32 = F(rtwp::kRad32), *m32 = F(rtwp::kMat32), *t32 = F(rtwp::kTg32);
  for (uint32_t pos = 0; pos < n; ++pos) {
    const rtw_sphere& s = sph[list_of[pos]];
    const float rf = (float)s.radius;
    const double want[8] = {s.c0[0], s.c0[1], s.c0[2], s.c1[0] - s.c0[0], s.c1[1] - s.c0[1], s.c1[2] - s.c0[2],
                            s.radius * s.radius, 1.0 / s.radius};
    for (int c = 0; c < 8; ++c) {
      CHECK(same_bits(s64[8 * pos + c], want[c]), "sph64[%u][%d] = %a, expected %a", pos, c, s64[8 * pos + c], want[c]);
      const float wf = c < 6 ? (float)want[c] : (c == 6 ? rf * rf : 1.0f / rf);  // r*r and 1/r computed in f32
      CHECK(same_bits(s32[8 * pos + c], wf), "sph32[%u][%d] = %a, expected %a", pos, c, s32[8 * pos + c], wf);
    }
    CHECK(same_bits(r64[pos], s.radius) && same_bits(r32[pos], rf), "radius of position %u", pos);
  }
  for (int c = 0; c < 8; ++c)
    CHECK(same_bits(s64[8 * n + c], 0.0) && same_bits(s32[8 * n + c], 0.0f), "sph padding record, field %d", c);
  const uint32_t* kind = U(rtwp::kKind);
  for (uint32_t i = 0; i < nm; ++i) {
    const rtw_material& m = mats[i];
    const bool diel = m.kind == RTW_DIELECTRIC;
    double wd[8] = {m.albedo[0], m.albedo[1], m.albedo[2], m.albedo_odd[0], m.albedo_odd[1], m.albedo_odd[2],
                    diel ? 1.0 / m.ir : m.fuzz, m.ir};
    float wf[8];
    for (int c = 0; c < 8; ++c) wf[c] = (float)wd[c];
    if (diel) {  // ratio and Schlick's r0^2 (front: RN(1/ir), back: ir) with each precision's own operations
      wf[6] = 1.0f / (float)m.ir;
      const double rd[2] = {wd[6], m.ir};
      const float rf[2] = {wf[6], (float)m.ir};
      for (int f = 0; f < 2; ++f) {
        const double r0d = (1.0 - rd[f]) / (1.0 + rd[f]);
        const float r0f = (1.0f - rf[f]) / (1.0f + rf[f]);
        wd[f] = r0d * r0d, wf[f] = r0f * r0f;
      }
    }
    for (int c = 0; c < 8; ++c)
      CHECK(same_bits(m64[8 * i + c], wd[c]) && same_bits(m32[8 * i + c], wf[c]), "material %u field %d: %a / %a", i, c,
            m64[8 * i + c], m32[8 * i + c]);
    CHECK(kind[i] == m.kind, "kind[%u]", i);
  }
  for (uint32_t g = 0; g < groups.size(); ++g) {
    const double t0 = groups[g].first, t1 = groups[g].second;
    const float f0 = (float)t0, f1 = (float)t1;
    CHECK(same_bits(t64[4 * g], t0) && same_bits(t64[4 * g + 1], t1) && same_bits(t64[4 * g + 2], 1.0 / (t1 - t0)) &&
              same_bits(t64[4 * g + 3], 0.0),
          "tg64[%u]", g);
    CHECK(same_bits(t32[4 * g], f0) && same_bits(t32[4 * g + 1], f1) && same_bits(t32[4 * g + 2], 1.0f / (f1 - f0)) &&
              same_bits(t32[4 * g + 3], 0.0f),
          "tg32[%u]", g);
  }

  // ---- pretest pair records over the narrow spheres (static narrow, then moving narrow)
  std::vector<uint32_t> narrow;  // narrow index -> table position
  for (uint32_t pos = end[0]; pos < end[1]; ++pos) narrow.push_back(pos);
  const uint32_t n_sn = (uint32_t)narrow.size();
  for (uint32_t pos = end[2]; pos < n; ++pos) narrow.push_back(pos);
  const uint32_t nn = (uint32_t)narrow.size(), nn_pad = (nn + 31u) / 32u * 32u;
  CHECK(k.nn == nn && k.nn_pad == nn_pad && k.n_sn == n_sn, "nn %u nn_pad %u n_sn %u, expected %u %u %u", k.nn, k.nn_pad,
        k.n_sn, nn, nn_pad, n_sn);
  if (k.nn != nn || k.nn_pad != nn_pad) return;
  std::vector<Slot> slot_of(nn);  // by narrow index
  double cmax_need = 0.0, rho_need = 1.0;
  const float* cull = F(rtwp::kCull);
  const uint32_t* cull_tg = U(rtwp::kCullTg);
  auto record_matches = [&](const float* q, uint32_t j) {  // q: a slot's 7 floats at stride 2
    const rtw_sphere& s = sph[list_of[narrow[j]]];
    const float rf = (float)s.radius;
    bool ok = same_bits(q[12], -(rf * rf));
    for (int c = 0; c < 3; ++c)
      ok = ok && same_bits(q[2 * c], (float)s.c0[c]) && same_bits(q[2 * (3 + c)], -(float)(s.c1[c] - s.c0[c]));
    return ok;
  };
  for (uint32_t j = 0; j < nn; ++j) {
    const rtw_sphere& s = sph[list_of[narrow[j]]];
    CHECK(record_matches(cull + 16 * (j / 2) + (j & 1), j), "pair record of narrow sphere %u", j);
    slot_of[j] = {true, s.moving != 0, tgroup[list_of[narrow[j]]], -(float)(s.c1[0] - s.c0[0]), -(float)(s.c1[2] - s.c0[2])};
    double c_inf = 0.0, d_inf = 0.0;
    for (int c = 0; c < 3; ++c) c_inf = std::fmax(c_inf, std::fabs(s.c0[c])), d_inf = std::fmax(d_inf, std::fabs(s.c1[c] - s.c0[c]));
    cmax_need = std::fmax(cmax_need, c_inf + d_inf);
    rho_need = std::fmax(rho_need, 2.0 * s.radius * s.radius + 1.0);
  }
  for (uint32_t j = nn; j < nn_pad; ++j)
    for (int c = 0; c < 7; ++c) CHECK(cull[16 * (j / 2) + (j & 1) + 2 * c] == 0.0f, "padding slot %u field %d", j, c);
  for (uint32_t p = 0; p < nn_pad / 2; ++p) {
    const Slot a = 2 * p < nn ? slot_of[2 * p] : Slot{}, b = 2 * p + 1 < nn ? slot_of[2 * p + 1] : Slot{};
    const uint32_t want = expected_tg(a, b, false);
    CHECK(cull_tg[p] == want, "cull_tg[%u] = %x, expected %x", p, cull_tg[p], want);
  }
  CHECK((double)k.cmax >= cmax_need && (double)k.rho >= rho_need, "cmax %a < %a or rho %a < %a", k.cmax, cmax_need, k.rho,
        rho_need);
  CHECK(k.cull_on == ((nn > 0 && k.cmax <= rtwc::kCmaxLimit) ? 1u : 0u), "cull_on %u", k.cull_on);

  // ---- clusters: slot tables and bounding spheres
  const uint32_t n_clusters = (nn + CS - 1) / CS, n_slots = CS * n_clusters;
  CHECK(k.n_clusters == n_clusters, "n_clusters %u, expected %u", k.n_clusters, n_clusters);
  if (k.n_clusters != n_clusters) return;
  const float *ccull = F(rtwp::kCcull), *cclus = F(rtwp::kCclus);
  const uint32_t *ccull_tg = U(rtwp::kCcullTg), *cpos = U(rtwp::kCpos), *cvalid = U(rtwp::kCvalid);
  std::vector<uint32_t> narrow_of(n, ~0u);  // table position -> narrow index
  for (uint32_t j = 0; j < nn; ++j) narrow_of[narrow[j]] = j;
  std::vector<uint32_t> uses(nn, 0u);
  std::vector<Slot> cslot(n_slots);
  double cmax_cl_need = 0.0, rho_cl_need = 1.0;
  for (uint32_t c = 0; c < n_clusters; ++c) {
    double mc0[CS][3], mdc[CS][3], mr[CS];
    int members = 0;
    bool seen_moving = false, seen_dummy = false;
    for (uint32_t i = 0; i < CS; ++i) {
      const uint32_t sl = CS * c + i;
      const float* q = ccull + 16 * (sl / 2) + (sl & 1);
      const bool real = !same_bits(q[12], 3e38f);
      const bool bit = (cvalid[2 * (sl / 64) + ((sl % 64) >> 5)] >> (31u - (sl & 31u))) & 1u;
      CHECK(bit == real, "cvalid of slot %u: %d, record says %d", sl, (int)bit, (int)real);
      if (!real) {
        seen_dummy = true;
        CHECK(cpos[sl] == 0u, "cpos of dummy slot %u = %u", sl, cpos[sl]);
        for (int f = 0; f < 6; ++f) CHECK(q[2 * f] == 0.0f, "dummy slot %u field %d", sl, f);
        continue;
      }
      CHECK(!seen_dummy, "real slot %u after a dummy", sl);
      const uint32_t j = cpos[sl] < n ? narrow_of[cpos[sl]] : ~0u;
      CHECK(j != ~0u, "cpos[%u] = %u is no narrow sphere's position", sl, cpos[sl]);
      if (j == ~0u) continue;
      ++uses[j];
      CHECK(record_matches(q, j), "slot %u does not hold the pair record of its member %u", sl, j);
      for (int f = 0; f < 7; ++f)
        CHECK(same_bits(q[2 * f], cull[16 * (j / 2) + (j & 1) + 2 * f]), "slot %u field %d differs from cull", sl, f);
      cslot[sl] = slot_of[j];
      CHECK(!(seen_moving && !cslot[sl].moving), "static member at slot %u after a moving one", sl);
      seen_moving = seen_moving || cslot[sl].moving;
      const rtw_sphere& s = sph[list_of[narrow[j]]];
      for (int a = 0; a < 3; ++a) mc0[members][a] = s.c0[a], mdc[members][a] = s.c1[a] - s.c0[a];
      mr[members++] = s.radius;
    }
    CHECK(members > 0, "cluster %u is empty", c);
    if (!members) continue;
    float cf[3], rf;
    rtwc::cluster_sphere(mc0, mdc, mr, members, cf, rf);
    const float* q = cclus + 16 * (c / 2) + (c & 1);
    bool ok = same_bits(q[12], -(rf * rf));
    for (int a = 0; a < 3; ++a) ok = ok && same_bits(q[2 * a], cf[a]) && q[2 * (3 + a)] == 0.0f;
    CHECK(ok, "bounding record of cluster %u", c);
    for (int a = 0; a < 3; ++a) cmax_cl_need = std::fmax(cmax_cl_need, std::fabs((double)cf[a]));
    rho_cl_need = std::fmax(rho_cl_need, 2.0 * (double)rf * (double)rf + 1.0);
  }
  for (uint32_t j = 0; j < nn; ++j) CHECK(uses[j] == 1u, "narrow sphere %u occupies %u slots", j, uses[j]);
  for (uint32_t sl = n_slots; sl < (n_slots + 63u) / 64u * 64u; ++sl)
    CHECK(!((cvalid[2 * (sl / 64) + ((sl % 64) >> 5)] >> (31u - (sl & 31u))) & 1u), "cvalid bit of slot %u past the end", sl);
  for (uint32_t p = 0; p < n_slots / 2; ++p) {
    const uint32_t want = expected_tg(cslot[2 * p], cslot[2 * p + 1], true);
    CHECK(ccull_tg[p] == want, "ccull_tg[%u] = %x, expected %x", p, ccull_tg[p], want);
  }
  CHECK(k.cmax_all >= k.cmax && (double)k.cmax_all >= cmax_cl_need && (double)k.rho_c >= rho_cl_need,
        "cmax_all %a (cmax %a, centres %a), rho_c %a (needs %a)", k.cmax_all, k.cmax, cmax_cl_need, k.rho_c, rho_cl_need);
  CHECK(k.cluster_ok == ((n_clusters > 0 && k.cull_on && k.cmax_all <= rtwc::kCmaxLimit) ? 1u : 0u), "cluster_ok %u",
        k.cluster_ok);
}

int g_scenes = 0;
void run(const char* name, const std::vector<rtw_sphere>& sph, const std::vector<rtw_material>& mats, const char* dump_dir) {
  rtwp::ScenePack k;
  std::string msg;
  const int st = rtwp::pack_scene(sph.data(), (uint32_t)sph.size(), mats.data(), (uint32_t)mats.size(), k, msg);
  g_scene = name;
  ++g_scenes;
  CHECK(st == RTW_OK, "pack_scene: %d %s", st, msg.c_str());
  if (st != RTW_OK) return;
  verify(name, sph, mats, k);
  if (dump_dir) {
    FILE* f = fopen((std::string(dump_dir) + "/" + name + ".blob").c_str(), "wb");
    if (!f || fwrite(k.blob.data(), 1, k.blob.size(), f) != k.blob.size()) CHECK(false, "cannot write the blob");
    if (f) fclose(f);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const char* dump_dir = argc > 1 ? argv[1] : nullptr;
  {
    std::vector<rtw_sphere> s(RTW_MAX_SPHERES);
    std::vector<rtw_material> m(RTW_MAX_SPHERES);
    uint32_t n = RTW_MAX_SPHERES, nm = RTW_MAX_SPHERES;
    if (rtw_cover_scene(42, s.data(), &n, m.data(), &nm, nullptr) != RTW_OK) return 2;
    s.resize(n), m.resize(nm);
    run("cover42", s, m, dump_dir);
  }
  const std::vector<rtw_material> mats = pack_inputs::five_materials();
  run("gen101", pack_inputs::generated_scene(101, true, 7), mats, dump_dir);
  run("empty", {}, mats, nullptr);
  run("one", pack_inputs::generated_scene(1, false, 3), mats, nullptr);
  run("movers_only", pack_inputs::generated_scene(10, false, 4, true), mats, nullptr);
  // 9 narrow spheres, 3 of them static: an odd narrow count, and the pair (2, 3) is mixed with a mover of group 1
  run("odd_narrow", pack_inputs::generated_scene(9, true, 5), mats, nullptr);
  run("slots_plus_one", pack_inputs::generated_scene(rtwk::kClusterSlots + 1, false, 6), mats, nullptr);
  printf("scenes %d checks %ld violations %ld\n", g_scenes, g_checks, g_viol);
  return g_viol ? 1 : 0;
}
