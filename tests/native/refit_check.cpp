// The host refit of a dynamic world (csrc/rtw_world_refit.cpp, the per-item
// steps of csrc/rtw_world_refit.hpp that the update kernels run too) against
// the packer and the descriptor:
//   1. a refit with the creation's own numbers reproduces every blob byte,
//      cull_cmax, cull_rho and the bounds;
//   2. after a random displacement every child box holds the f64 box
//      (rtw_world_box.hpp prim_box, the packer's statement) of each primitive
//      beneath it; the packed lower bounds are <= the plain ones, within 512
//      ulps, and their low bytes decode to compact_ref(ref); refs and order
//      are unchanged; the records are the packer's of the new numbers;
//   3. kCullBit follows the rule when a radius crosses 100 and when a centre
//      crosses 2^20, and the created bytes return after moving back;
//   4. the refit's world box is pack_world's of the updated description;
//   and rtwr::prim_box / lower_with_low8 give the bits of the packer's own.
//
// usage: refit_check WORLD.bin...  (descriptors dumped by tests/test_refit_host.py)
//   ->  "worlds W checks C violations V", exit 1 if V > 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rtw_cull.hpp"
#include "rtw_layout.hpp"
#include "rtw_world_box.hpp"
#include "rtw_world_pack.hpp"
#include "rtw_world_refit.hpp"

namespace {

long g_checks = 0, g_viol = 0;
const char* g_world = "";
#define CHECK(cond, ...)                           \
  do {                                             \
    ++g_checks;                                    \
    if (!(cond) && g_viol++ < 20) {                \
      fprintf(stderr, "%s: %s: ", g_world, #cond); \
      fprintf(stderr, __VA_ARGS__);                \
      fprintf(stderr, "\n");                       \
    }                                              \
  } while (0)

template <typename T>
bool same_bits(T a, T b) {
  return std::memcmp(&a, &b, sizeof(T)) == 0;
}

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uni(double lo, double hi) { return lo + (hi - lo) * ((double)(next() >> 11) * 0x1p-53); }
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
bool load(const char* path, World& w) {  // tests/test_refit_host.py dump_desc
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

uint32_t ulps_below(float lo, float ref) {  // ulps from lo up to ref (lo <= ref)
  auto key = [](float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return (b & 0x80000000u) ? (int64_t)0 - (int64_t)(b & 0x7FFFFFFFu) : (int64_t)b;
  };
  return (uint32_t)std::min<int64_t>(key(ref) - key(lo), 0xFFFFFFFFll);
}

struct Tables {
  const rtwp::WorldPack* k;
  const rtwp::RefitPack* r;
  const float* nodes() const { return reinterpret_cast<const float*>(k->blob.data() + k->o_node); }
  const float* plain() const { return reinterpret_cast<const float*>(r->blob.data() + r->o_plain); }
  const double* prim() const { return reinterpret_cast<const double*>(k->blob.data() + k->o_prim); }
  const uint32_t* order() const { return reinterpret_cast<const uint32_t*>(k->blob.data() + k->o_order); }
  uint32_t ref(uint32_t n, int c) const { return rtwr::ld_u32(nodes() + (size_t)rtwk::kNodeWords * n, 12 + c); }
  uint32_t cull_bits() const {
    uint32_t s = 0;
    for (uint32_t n = 0; n < k->n_nodes; ++n)
      for (int c = 0; c < 2; ++c) s += (ref(n, c) & rtwk::kLeafBit) && (ref(n, c) & rtwk::kCullBit);
    return s;
  }
};

// check 2 (and the records): the refitted tables of `w`'s numbers; `k0`: as created
Box verify_node(const World& w, const Tables& t, const rtwp::WorldPack& k0, const std::vector<uint32_t>& list_of, uint32_t n) {
  Box all;
  const float* nd = t.nodes() + (size_t)rtwk::kNodeWords * n;
  const float* pl = t.plain() + (size_t)12 * n;
  const float* nd0 = reinterpret_cast<const float*>(k0.blob.data() + k0.o_node) + (size_t)rtwk::kNodeWords * n;
  for (int c = 0; c < 2; ++c) {
    const uint32_t ref = t.ref(n, c), ref0 = rtwr::ld_u32(nd0, 12 + c);
    const uint32_t mask = (ref & rtwk::kLeafBit) ? ~rtwk::kCullBit : ~0u;
    CHECK((ref & mask) == (ref0 & mask), "node %u child %d: ref %x was %x", n, c, ref, ref0);
    Box sub;
    if (ref & rtwk::kLeafBit) {
      const uint32_t first = ref & 0x7FFFFFu, cnt = (ref >> 23) & rtwk::kLeafCountMask;
      for (uint32_t pos = first; pos < first + cnt; ++pos) {
        const rtw_prim& p = w.prims[list_of[pos]];
        sub.grow(prim_box(p, p.xform >= 0 ? &w.xforms[p.xform] : nullptr));
      }
    } else {
      sub = verify_node(w, t, k0, list_of, ref);
    }
    uint32_t v = 0;
    for (int a = 0; a < 3; ++a) {
      const float lo = nd[2 * a + c], hi = nd[6 + 2 * a + c], plo = pl[2 * a + c], phi = pl[6 + 2 * a + c];
      CHECK(!(sub.lo[a] <= sub.hi[a]) || ((double)plo <= sub.lo[a] && (double)phi >= sub.hi[a]),
            "node %u child %d axis %d: plain [%a, %a] does not hold [%a, %a]", n, c, a, plo, phi, sub.lo[a], sub.hi[a]);
      CHECK(same_bits(hi, phi), "node %u child %d axis %d: upper bound %a, plain %a", n, c, a, hi, phi);
      if (t.k->packed) {
        CHECK(lo <= plo && ulps_below(lo, plo) < 512u, "node %u child %d axis %d: packed %a, plain %a (%u ulps)", n, c, a, lo,
              plo, ulps_below(lo, plo));
        v |= (rtwr::f32_bits(lo) & 255u) << (8 * a);
      } else {
        CHECK(same_bits(lo, plo), "node %u child %d axis %d: lower bound %a, plain %a", n, c, a, lo, plo);
      }
    }
    if (t.k->packed) CHECK(v == rtwp::compact_ref(ref), "node %u child %d: gathered ref %x, compact_ref %x", n, c, v, rtwp::compact_ref(ref));
    all.grow(sub);
  }
  return all;
}

void verify_refit(const World& w, const rtwp::WorldPack& k, const rtwp::RefitPack& r, const rtwp::WorldPack& k0) {
  const Tables t{&k, &r};
  const uint32_t n = k.n_prims;
  CHECK(std::memcmp(k.blob.data() + k.o_order, k0.blob.data() + k0.o_order, 4 * (size_t)n) == 0, "order changed");
  CHECK(k.blob.size() == k0.blob.size(), "blob size changed");
  std::vector<uint32_t> list_of(n);
  for (uint32_t li = 0; li < n; ++li) list_of[t.order()[li]] = li;
  // records and everything outside the updated tables: the packer's of the updated description
  const rtw_world_desc d = w.desc();
  rtwp::WorldPack fresh;
  std::string msg;
  const int st = rtwp::pack_world(&d, w.flags, false, fresh, msg);
  CHECK(st == RTW_OK, "pack_world of the updated description: %s", msg.c_str());
  if (st != RTW_OK) return;
  for (uint32_t li = 0; li < n; ++li) {  // (a fresh world may store the primitives elsewhere: compare by list index)
    const uint32_t pf = reinterpret_cast<const uint32_t*>(fresh.blob.data() + fresh.o_order)[li];
    const double* a = t.prim() + (size_t)rtwk::kWorldRec * t.order()[li];
    const double* b = reinterpret_cast<const double*>(fresh.blob.data() + fresh.o_prim) + (size_t)rtwk::kWorldRec * pf;
    CHECK(std::memcmp(a, b, rtwk::kWorldRec * 8) == 0, "record of list index %u differs from the fresh world's", li);
  }
  CHECK(fresh.o_node == k.o_node && std::memcmp(fresh.blob.data() + fresh.o_xform, k.blob.data() + k.o_xform, k.o_node - k.o_xform) == 0,
        "xform ... pixel tables differ from the fresh world's");
  for (int a = 0; a < 3; ++a)  // check 4
    CHECK(fresh.bounds_lo[a] == k.bounds_lo[a] && fresh.bounds_hi[a] == k.bounds_hi[a], "bounds axis %d: [%a, %a], fresh [%a, %a]", a,
          k.bounds_lo[a], k.bounds_hi[a], fresh.bounds_lo[a], fresh.bounds_hi[a]);
  if (k.n_nodes) verify_node(w, t, k0, list_of, 0);
  // every leaf with the bit qualifies by the packer's rule on the new numbers, and Cmax / rho cover it
  for (uint32_t nd = 0; nd < k.n_nodes; ++nd)
    for (int c = 0; c < 2; ++c) {
      const uint32_t ref = t.ref(nd, c);
      if (!(ref & rtwk::kLeafBit) || !(ref & rtwk::kCullBit)) continue;
      const uint32_t first = ref & 0x7FFFFFu, cnt = (ref >> 23) & rtwk::kLeafCountMask;
      const float* q = reinterpret_cast<const float*>(k.blob.data() + k.o_cull) + (size_t)16 * first;
      for (uint32_t j = 0; j < cnt; ++j) {
        const rtw_prim& p = w.prims[list_of[first + j]];
        const bool el = p.xform < 0 && std::fabs(p.a[6]) < 100.0 &&
                        (p.kind == RTW_PRIM_SPHERE || (p.kind == RTW_PRIM_MOVING_SPHERE && p.a[7] == 0.0 && p.a[8] == 1.0));
        CHECK(el, "kCullBit on a leaf whose sphere %u does not qualify", list_of[first + j]);
        const float rf = (float)p.a[6];
        bool ok = same_bits(q[12 + j], -(rf * rf));
        double c_inf = 0, d_inf = 0;
        for (int a = 0; a < 3; ++a) {
          const double dc = p.kind == RTW_PRIM_MOVING_SPHERE ? p.a[3 + a] - p.a[a] : 0.0;
          ok = ok && same_bits(q[2 * a + j], (float)p.a[a]) && same_bits(q[2 * (3 + a) + j], -(float)dc);
          c_inf = std::fmax(c_inf, std::fabs(p.a[a])), d_inf = std::fmax(d_inf, std::fabs(dc));
        }
        CHECK(ok, "pretest record of sphere %u", list_of[first + j]);
        CHECK((double)k.cull_cmax >= c_inf + d_inf && (double)k.cull_rho >= 2.0 * p.a[6] * p.a[6] + 1.0 && k.cull_cmax <= rtwc::kCmaxLimit,
              "cull_cmax %a / cull_rho %a do not cover sphere %u", k.cull_cmax, k.cull_rho, list_of[first + j]);
      }
    }
}

void same_world(const rtwp::WorldPack& k, const rtwp::WorldPack& k0, const char* what) {
  CHECK(k.blob == k0.blob, "%s: the blob differs from the created one", what);
  CHECK(same_bits(k.cull_cmax, k0.cull_cmax) && same_bits(k.cull_rho, k0.cull_rho), "%s: cull_cmax %a (created %a), cull_rho %a (%a)", what,
        k.cull_cmax, k0.cull_cmax, k.cull_rho, k0.cull_rho);
  for (int a = 0; a < 3; ++a)
    CHECK(k.bounds_lo[a] == k0.bounds_lo[a] && k.bounds_hi[a] == k0.bounds_hi[a], "%s: bounds axis %d", what, a);
}

void run(const char* path, uint64_t seed) {
  g_world = path;
  World w;
  const bool loaded = load(path, w);
  CHECK(loaded, "cannot read the descriptor");
  if (!loaded) return;
  const World w0 = w;
  rtw_world_desc d = w.desc();
  rtwp::WorldPack k0, k;
  std::string msg;
  const int st = rtwp::pack_world(&d, w.flags, false, k0, msg);
  CHECK(st == RTW_OK, "pack_world: %s", msg.c_str());
  if (st != RTW_OK) return;
  k = k0;
  rtwp::RefitPack r;
  rtwp::make_refit(&d, k, r);
  const rtwp::RefitPack r0 = r;
  std::vector<double> a, xv;

  // the shared arithmetic against the packer's own statements
  Rng g{seed};
  for (size_t i = 0; i < w.prims.size(); ++i) {
    const rtw_prim& p = w.prims[i];
    const Box b = prim_box(p, p.xform >= 0 ? &w.xforms[p.xform] : nullptr);
    double lo[3], hi[3];
    rtwr::prim_box(p.kind, p.a, p.xform >= 0 ? r.xf_header[p.xform] : 0u, p.xform >= 0 ? &w.xforms[p.xform].v[0][0] : p.a, lo, hi);
    CHECK(std::memcmp(lo, b.lo, 24) == 0 && std::memcmp(hi, b.hi, 24) == 0, "rtwr::prim_box of prim %zu differs from rtw_world_box.hpp's", i);
  }
  for (int i = 0; i < 20000; ++i) {
    const uint32_t bits = (uint32_t)g.next(), payload = (uint32_t)g.next() & 255u;
    float f = i < 8 ? (i & 1 ? -0.0f : 0.0f) : rtwr::bits_f32(bits);
    if (i >= 8 && i < 200) f = rtwr::bits_f32(bits & 0x800003FFu);  // zero, tiny and denormal values
    if (!std::isfinite(f)) continue;
    CHECK(same_bits(rtwr::lower_with_low8(f, payload), rtwp::pack_lower_with_low8(f, payload)), "lower_with_low8(%a, %u)", f, payload);
    const double x = (double)f * (1.0 + g.uni(-1e-9, 1e-9));
    float dn = (float)x, upf = (float)x;
    if ((double)dn > x) dn = std::nextafter(dn, -INFINITY);
    if ((double)upf < x) upf = std::nextafter(upf, INFINITY);
    CHECK(same_bits(rtwr::down(x), dn) && same_bits(rtwr::up(x), upf), "down / up of %a", x);
  }

  // 1. identity
  w.numbers(a, xv);
  CHECK(rtwp::refit_world(k, r, a.data(), xv.empty() ? nullptr : xv.data()) == RTW_OK, "identity refit refused: %s", r.msg.c_str());
  same_world(k, k0, "identity");
  CHECK(r.blob == r0.blob, "identity: the plain bounds differ from the created ones");

  // 2. + 4. a random displacement: every number that places a primitive, every transform
  for (rtw_prim& p : w.prims) {
    if (p.kind <= RTW_PRIM_MOVING_SPHERE) {
      const double s = std::fmin(std::fabs(p.a[6]), 5.0) * 3.0;
      for (int c = 0; c < 3; ++c) {
        const double dlt = g.uni(-s, s);
        p.a[c] += dlt, p.a[3 + c] += dlt + (p.kind == RTW_PRIM_MOVING_SPHERE ? g.uni(-0.3, 0.3) : 0.0);
      }
      p.a[6] *= g.uni(0.7, 1.3);
    } else {
      const double d0 = g.uni(-0.5, 0.5), d1 = g.uni(-0.5, 0.5);
      p.a[0] += d0, p.a[1] += d0 + g.uni(0.0, 0.2), p.a[2] += d1, p.a[3] += d1 + g.uni(0.0, 0.2), p.a[4] += g.uni(-0.5, 0.5);
    }
  }
  for (rtw_xform& x : w.xforms)
    for (uint32_t c = 0; c < x.n; ++c) {
      if (x.op[c] == RTW_XF_TRANSLATE) {
        for (int e = 0; e < 3; ++e) x.v[c][e] += g.uni(-1.0, 1.0);
      } else {
        x.v[c][2] += g.uni(-0.8, 0.8), x.v[c][0] = std::sin(x.v[c][2]), x.v[c][1] = std::cos(x.v[c][2]);
      }
    }
  w.numbers(a, xv);
  CHECK(rtwp::refit_world(k, r, a.data(), xv.empty() ? nullptr : xv.data()) == RTW_OK, "displacement refit refused: %s", r.msg.c_str());
  verify_refit(w, k, r, k0);
  // ... and back: the refit is a function of the numbers, not of the history
  w = w0;
  w.numbers(a, xv);
  CHECK(rtwp::refit_world(k, r, a.data(), xv.empty() ? nullptr : xv.data()) == RTW_OK, "refit back refused");
  same_world(k, k0, "moved back");

  // refusals leave everything as it was
  for (double bad : {(double)NAN, (double)INFINITY}) {
    if (a.empty()) break;
    a[0] = bad;
    CHECK(rtwp::refit_world(k, r, a.data(), nullptr) == RTW_EINVAL && !r.msg.empty(), "a non-finite centre was accepted");
    same_world(k, k0, "after a refusal");
    a[0] = w0.prims[0].a[0];
  }
  for (size_t i = 0; i < w.prims.size(); ++i)
    if (w.prims[i].kind == RTW_PRIM_MOVING_SPHERE) {
      a[9 * i + 8] = a[9 * i + 7];
      CHECK(rtwp::refit_world(k, r, a.data(), nullptr) == RTW_EINVAL, "time1 == time0 was accepted");
      same_world(k, k0, "after the shutter refusal");
      a[9 * i + 8] = w0.prims[i].a[8];
      break;
    }

  // 3. the pretest's rule
  const Tables t{&k, &r};
  const uint32_t bits0 = t.cull_bits();
  if (k.has_cull) {
    CHECK(bits0 > 0, "a pretest table without a kCullBit leaf");
    const uint32_t* mate = reinterpret_cast<const uint32_t*>(r.blob.data() + r.o_mate);
    uint32_t li = 0;
    while (li < k.n_prims && mate[li] == rtwr::kNone) ++li;
    CHECK(li < k.n_prims, "no candidate leaf");
    if (li < k.n_prims) {
      a[9 * li + 6] = 101.0;  // a radius across 100: exactly its leaf loses the bit
      CHECK(rtwp::refit_world(k, r, a.data(), nullptr) == RTW_OK, "radius refit refused");
      CHECK(t.cull_bits() == bits0 - 1, "radius 101: %u cull bits, %u before", t.cull_bits(), bits0);
      verify_refit([&] { World x = w0; x.prims[li].a[6] = 101.0; return x; }(), k, r, k0);
      a[9 * li + 6] = w0.prims[li].a[6];
      CHECK(rtwp::refit_world(k, r, a.data(), nullptr) == RTW_OK, "radius refit back refused");
      same_world(k, k0, "radius back");
      a[9 * li + 0] = 0x1p20 + 4.0;  // a centre across 2^20: every leaf loses it
      a[9 * li + 3] += 0x1p20 + 4.0 - w0.prims[li].a[0];
      CHECK(rtwp::refit_world(k, r, a.data(), nullptr) == RTW_OK, "far centre refit refused");
      CHECK(t.cull_bits() == 0 && k.cull_cmax > rtwc::kCmaxLimit, "far centre: %u cull bits, cull_cmax %a", t.cull_bits(), k.cull_cmax);
      a[9 * li + 0] = w0.prims[li].a[0], a[9 * li + 3] = w0.prims[li].a[3];
      CHECK(rtwp::refit_world(k, r, a.data(), nullptr) == RTW_OK, "far centre refit back refused");
      same_world(k, k0, "far centre back");
    }
  } else {
    CHECK(bits0 == 0, "kCullBit without a pretest table");
  }
}

}  // namespace

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) run(argv[i], 1000 + i);
  printf("worlds %d checks %ld violations %ld\n", argc - 1, g_checks, g_viol);
  return g_viol ? 1 : 0;
}
