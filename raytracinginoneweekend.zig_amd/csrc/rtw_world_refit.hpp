// rtw_world_refit.hpp — the arithmetic the world packer (rtw_world_pack.cpp),
// the host refit (rtw_world_refit.cpp) and the update kernels
// (rtw_world_update.hip) share, so that a refitted table and a packed one
// cannot drift: the prim record fill, a primitive's world-space box, outward
// rounding to f32, the ref bytes in the lower bounds, the leaf pretest record
// and eligibility, and the three per-item steps of an update (validate,
// record, node).  (rtw_world_box.hpp's prim_box and the packer's
// lower_with_low8 keep their own statements, whose text existing checks pin;
// tests/native/refit_check.cpp compares each with the one here, bit for bit.)
// Host and device; one IEEE operation per operator (the library builds with
// -ffp-contract=off); no arrays indexed at run time, so the kernels need no
// scratch.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rtw_layout.hpp"

#if defined(__HIPCC__)
#define RTWR_HD __host__ __device__ inline
#else
#define RTWR_HD inline
#endif

// The triangle's derived fields (rtw_tri.hpp, which defines it): declared here
// so that this header keeps standing on rtw_layout.hpp alone; a translation
// unit that packs, validates or commits primitives includes rtw_tri.hpp too.
namespace rtwtri {
RTWR_HD bool derive(const double* a, double n[3], double& h);
}

namespace rtwr {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kPartial = 11;  // doubles of a validation partial (struct Partial)
constexpr uint32_t kBlock = 256;   // lanes per workgroup of every update kernel

RTWR_HD double inf() { return __builtin_huge_val(); }
// std::min / std::max's choice on ties and NaNs (the first argument stays)
RTWR_HD double dmin(double a, double b) { return b < a ? b : a; }
RTWR_HD double dmax(double a, double b) { return a < b ? b : a; }
RTWR_HD float fmin32(float a, float b) { return b < a ? b : a; }
RTWR_HD float fmax32(float a, float b) { return a < b ? b : a; }
// total order on zeros (-0 < +0): a reduction's result does not depend on its order
RTWR_HD double tmin(double a, double b) { return (b < a || (b == a && __builtin_signbit(b))) ? b : a; }
RTWR_HD double tmax(double a, double b) { return (a < b || (a == b && __builtin_signbit(a))) ? b : a; }
RTWR_HD bool finite(double x) { return x - x == 0.0; }

RTWR_HD uint32_t f32_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
RTWR_HD float bits_f32(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}
RTWR_HD uint32_t ld_u32(const void* base, size_t word) {
  uint32_t u;
  __builtin_memcpy(&u, static_cast<const unsigned char*>(base) + 4 * word, 4);
  return u;
}
RTWR_HD void st_u32(void* base, size_t word, uint32_t u) {
  __builtin_memcpy(static_cast<unsigned char*>(base) + 4 * word, &u, 4);
}

// std::nextafter(f, -inf) / (f, +inf) on the bits
RTWR_HD float next_down(float f) {
  const uint32_t u = f32_bits(f);
  if (f != f || u == 0xFF800000u) return f;
  if ((u & 0x7FFFFFFFu) == 0u) return bits_f32(0x80000001u);
  return bits_f32((u & 0x80000000u) ? u + 1u : u - 1u);
}
RTWR_HD float next_up(float f) {
  const uint32_t u = f32_bits(f);
  if (f != f || u == 0x7F800000u) return f;
  if ((u & 0x7FFFFFFFu) == 0u) return bits_f32(0x00000001u);
  return bits_f32((u & 0x80000000u) ? u - 1u : u + 1u);
}
RTWR_HD float down(double x) {  // largest float <= x
  float f = (float)x;
  if ((double)f > x) f = next_down(f);
  return f;
}
RTWR_HD float up(double x) {  // smallest float >= x
  float f = (float)x;
  if ((double)f < x) f = next_up(f);
  return f;
}

// The largest float <= f whose low byte is `payload` (rtw_world_pack.cpp has
// the packer's statement and the reason; tests/native/refit_check.cpp holds
// the two together).
RTWR_HD float lower_with_low8(float f, uint32_t payload) {
  const uint32_t b = f32_bits(f);
  if (!(b & 0x80000000u) && b >= 256u && f != 0.0f) {
    uint32_t c = (b & ~255u) | payload;
    if (c > b) c -= 256u;
    return bits_f32(c);
  }
  const uint32_t m = b & 0x7FFFFFFFu;
  uint32_t c = (m & ~255u) | payload;
  if (c < m) c += 256u;
  return bits_f32(c | 0x80000000u);
}

// A child ref (node words 12-13) as the 24 bits the per-lane walk gathers from
// the low bytes of the child's three lower bounds: an interior node index
// < 2^23, or 0x800000 | (count - 1) << 22 | first primitive < 2^22.
RTWR_HD uint32_t compact_ref(uint32_t r) {
  if (r < rtwk::kLeafBit) return r;
  return 0x800000u | ((((r >> 23) & rtwk::kLeafCountMask) - 1u) << 22) | (r & 0x7FFFFFu);
}

// Doubles 0-10 of a primitive's device record from its a[9] (kind: rtw_prim_kind).
RTWR_HD void fill_record(uint32_t kind, const double* a, double r[11]) {
  for (int k = 0; k < 11; ++k) r[k] = 0.0;
  if (kind <= 1u) {
    r[0] = a[0], r[1] = a[1], r[2] = a[2];
    if (kind == 1u) {
      r[3] = a[3] - a[0], r[4] = a[4] - a[1], r[5] = a[5] - a[2];  // center1.sub(center0)
      r[7] = a[7];
      r[8] = a[8] - a[7];  // time1 - time0
      r[10] = 1.0 / r[8];  // its reciprocal (Markstein division in the kernel)
    }
    r[6] = a[6];
    r[9] = a[6] * a[6];  // sphere.radius * sphere.radius
  } else {
    r[0] = a[0], r[1] = a[1], r[2] = a[2], r[3] = a[3], r[4] = a[4];
    r[5] = a[1] - a[0];
    r[6] = a[3] - a[2];
  }
}

// A triangle's record (kind 5, rtw_tri.hpp): its vertices and the derived n, h
// in doubles 0-10, 12, 13 of r (r[11], the per-lane walk's kind copy, is not
// touched).  false: degenerate or not finite.
RTWR_HD bool fill_record_tri(const double* a, double r[14]) {
  for (int k = 0; k < 9; ++k) r[k] = a[k];
  double n[3], h;
  const bool ok = rtwtri::derive(a, n, h);
  r[9] = n[0], r[10] = n[1], r[12] = n[2], r[13] = h;  // rtwtri::kNx, kNy, kNz, kH
  return ok;
}

// Header word of a transform record: n | op[k] << (8 + 4 k).
RTWR_HD uint32_t xform_ops(uint32_t h) { return h & 0xFFu; }
RTWR_HD uint32_t xform_op(uint32_t h, int k) { return (h >> (8 + 4 * k)) & 0xFu; }

// World-space bounding box of a primitive: the reference's boudingBox
// (hittable.zig:133-143 sphere, :203-217 moving sphere over the camera
// shutter [0, 1], :304-317 / :359-372 / :414-427 rects padded by 1e-4)
// through its Translate / RotateY chain (:493-501, :514-556).  xf_h: the
// chain's header word (0: none), v: its values, three per op.
RTWR_HD void prim_box(uint32_t kind, const double* a, uint32_t xf_h, const double* v, double lo[3], double hi[3]) {
  lo[0] = lo[1] = lo[2] = inf();
  hi[0] = hi[1] = hi[2] = -inf();
  if (kind <= 1u) {
    const double r = __builtin_fabs(a[6]);
    for (int s = 0; s < 2; ++s) {
      if (s == 1 && kind != 1u) break;
      double c0 = a[0], c1 = a[1], c2 = a[2];
      if (kind == 1u) {
        const double f = ((double)s - a[7]) / (a[8] - a[7]);
        c0 = a[0] + (a[3] - a[0]) * f;
        c1 = a[1] + (a[4] - a[1]) * f;
        c2 = a[2] + (a[5] - a[2]) * f;
      }
      lo[0] = dmin(lo[0], c0 - r), hi[0] = dmax(hi[0], c0 + r);
      lo[1] = dmin(lo[1], c1 - r), hi[1] = dmax(hi[1], c1 + r);
      lo[2] = dmin(lo[2], c2 - r), hi[2] = dmax(hi[2], c2 + r);
    }
  } else if (kind == 5u) {  // triangle: its vertices' box, padded by 1e-4 on every axis as a rect's plane is
    lo[0] = dmin(dmin(a[0], a[3]), a[6]) - 0.0001, hi[0] = dmax(dmax(a[0], a[3]), a[6]) + 0.0001;
    lo[1] = dmin(dmin(a[1], a[4]), a[7]) - 0.0001, hi[1] = dmax(dmax(a[1], a[4]), a[7]) + 0.0001;
    lo[2] = dmin(dmin(a[2], a[5]), a[8]) - 0.0001, hi[2] = dmax(dmax(a[2], a[5]), a[8]) + 0.0001;
  } else {
    const double k0 = a[4] - 0.0001, k1 = a[4] + 0.0001;
    if (kind == 2u) {  // XY: x, y, k on z
      lo[0] = a[0], hi[0] = a[1], lo[1] = a[2], hi[1] = a[3], lo[2] = k0, hi[2] = k1;
    } else if (kind == 3u) {  // XZ: x, z, k on y
      lo[0] = a[0], hi[0] = a[1], lo[2] = a[2], hi[2] = a[3], lo[1] = k0, hi[1] = k1;
    } else {  // YZ: y, z, k on x
      lo[1] = a[0], hi[1] = a[1], lo[2] = a[2], hi[2] = a[3], lo[0] = k0, hi[0] = k1;
    }
  }
  const int n = (int)xform_ops(xf_h);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = (int)rtwk::kMaxXfOps - 1; i >= 0; --i) {
    if (i >= n) continue;
    const double v0 = v[3 * i], v1 = v[3 * i + 1], v2 = v[3 * i + 2];
    if (xform_op(xf_h, i) == 0u) {  // RTW_XF_TRANSLATE
      lo[0] += v0, hi[0] += v0, lo[1] += v1, hi[1] += v1, lo[2] += v2, hi[2] += v2;
    } else {  // RTW_XF_ROTATE_Y: v = {sin, cos, angle}
      const double sn = v0, cs = v1;
      double nl0 = inf(), nl1 = inf(), nl2 = inf(), nh0 = -inf(), nh1 = -inf(), nh2 = -inf();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int c = 0; c < 8; ++c) {
        const double x = (c & 1) ? hi[0] : lo[0], y = (c & 2) ? hi[1] : lo[1], z = (c & 4) ? hi[2] : lo[2];
        const double q0 = cs * x + sn * z, q1 = y, q2 = -sn * x + cs * z;
        nl0 = dmin(nl0, q0), nh0 = dmax(nh0, q0);
        nl1 = dmin(nl1, q1), nh1 = dmax(nh1, q1);
        nl2 = dmin(nl2, q2), nh2 = dmax(nh2, q2);
      }
      lo[0] = nl0, lo[1] = nl1, lo[2] = nl2, hi[0] = nh0, hi[1] = nh1, hi[2] = nh2;
    }
  }
}

// A sphere a leaf's pretest record may hold (rtw_world_pack.cpp "Leaf pretest
// records"): untransformed, narrow, static or moving over the shutter [0, 1].
// meta0: kind | (xform + 1) << 8, the record's first meta word.
RTWR_HD bool eligible(uint32_t meta0, const double* a) {
  const uint32_t kind = meta0 & 0xFFu;
  if ((meta0 >> 8) != 0u || !(__builtin_fabs(a[6]) < 100.0)) return false;
  return kind == 0u || (kind == 1u && a[7] == 0.0 && a[8] == 1.0);
}

// Sphere j (0 or 1) of a leaf's pretest record at q = cull + 16 * first, from
// the sphere's record doubles r: lane j of each float pair.
RTWR_HD void fill_cull(float* q, uint32_t j, const double* r) {
  q[0 + j] = (float)r[0], q[2 + j] = (float)r[1], q[4 + j] = (float)r[2];
  q[6 + j] = -(float)r[3], q[8 + j] = -(float)r[4], q[10 + j] = -(float)r[5];
  const float rf = (float)r[6];
  q[12 + j] = -(rf * rf);
}

// ------------------------------------------------------------- an update --
// What one update reads and writes: the world's tables, the refit tables made
// at creation (rtw_world_refit.cpp), and the caller's numbers.
struct View {
  double* prim;           // world tables (rtwk::WorldView's)
  double* xform;
  float* node;
  const uint32_t* order;  // list index -> stored position
  float* cull;
  float* plain;               // 12 f32 per node: the bounds before pack_refs
  const uint32_t* by_height;  // node indices, by height
  const uint32_t* heights;    // height of by_height[i]
  const uint32_t* cand;       // per node: bit c = child c is a leaf whose spheres all qualified at creation
  const uint32_t* mate;       // per list index: the other sphere of its candidate leaf (itself if alone), kNone if in none
  const double* a;            // input: n_prims x 9, list order
  const double* xv;           // input: n_xforms x kMaxXfOps x 3, or NULL (the table's values stay)
  uint32_t n_prims, n_xforms, n_nodes;
  uint32_t packed;     // the tree carries its refs in the lower bounds
  uint32_t has_table;  // the world was created with a pretest table
  uint32_t cull_on;    // this update's Cmax is within rtwc::kCmaxLimit
  uint32_t has_tri;    // the world holds triangles (feature bit 64): records carry doubles 12-13
};

RTWR_HD const double* xform_vals(const View& V, uint32_t xi) {
  return V.xv ? V.xv + (size_t)3 * rtwk::kMaxXfOps * xi : V.xform + (size_t)rtwk::kWorldRec * xi + 4;
}
RTWR_HD uint32_t prim_meta0(const View& V, uint32_t pos) { return ld_u32(V.prim + (size_t)rtwk::kWorldRec * pos + 14, 0); }
RTWR_HD uint32_t prim_list_index(const View& V, uint32_t pos) { return ld_u32(V.prim + (size_t)rtwk::kWorldRec * pos + 14, 2); }
RTWR_HD void box_of(const View& V, uint32_t meta0, uint32_t li, double lo[3], double hi[3]) {
  const uint32_t xf = meta0 >> 8;
  const uint32_t h = xf ? ld_u32(V.xform + (size_t)rtwk::kWorldRec * (xf - 1u), 0) : 0u;
  prim_box(meta0 & 0xFFu, V.a + (size_t)9 * li, h, xf ? xform_vals(V, xf - 1u) : V.a, lo, hi);
}

// What validation reduces: the f64 world box, the pretest's maxima, violations.
struct Partial {
  double lo[3], hi[3];
  double cc, cd, rho;    // max |c0|, max |c1 - c0|, max 2 r^2 + 1 over the pretested spheres
  double bad, first_bad; // violations, the smallest index among them (primitives, then n_prims + transform)
};
static_assert(sizeof(Partial) == kPartial * sizeof(double), "Partial is kPartial doubles");
RTWR_HD void partial_init(Partial& p) {
  p.lo[0] = p.lo[1] = p.lo[2] = inf();
  p.hi[0] = p.hi[1] = p.hi[2] = -inf();
  p.cc = 0.0, p.cd = 0.0, p.rho = 1.0, p.bad = 0.0, p.first_bad = inf();
}
RTWR_HD void partial_store(const Partial& p, double* d) {
  d[0] = p.lo[0], d[1] = p.lo[1], d[2] = p.lo[2], d[3] = p.hi[0], d[4] = p.hi[1], d[5] = p.hi[2];
  d[6] = p.cc, d[7] = p.cd, d[8] = p.rho, d[9] = p.bad, d[10] = p.first_bad;
}
RTWR_HD void partial_load(Partial& p, const double* d) {
  p.lo[0] = d[0], p.lo[1] = d[1], p.lo[2] = d[2], p.hi[0] = d[3], p.hi[1] = d[4], p.hi[2] = d[5];
  p.cc = d[6], p.cd = d[7], p.rho = d[8], p.bad = d[9], p.first_bad = d[10];
}
RTWR_HD void partial_fold(Partial& p, const Partial& q) {
  p.lo[0] = tmin(p.lo[0], q.lo[0]), p.lo[1] = tmin(p.lo[1], q.lo[1]), p.lo[2] = tmin(p.lo[2], q.lo[2]);
  p.hi[0] = tmax(p.hi[0], q.hi[0]), p.hi[1] = tmax(p.hi[1], q.hi[1]), p.hi[2] = tmax(p.hi[2], q.hi[2]);
  p.cc = dmax(p.cc, q.cc), p.cd = dmax(p.cd, q.cd), p.rho = dmax(p.rho, q.rho);
  p.bad = p.bad + q.bad;  // (whole numbers < 2^53: exact in any order)
  p.first_bad = dmin(p.first_bad, q.first_bad);
}

// Validation of list index i: reads the input only.
RTWR_HD void validate_prim(const View& V, uint32_t i, Partial& p) {
  const uint32_t meta0 = prim_meta0(V, V.order[i]), kind = meta0 & 0xFFu;
  const double* a = V.a + (size_t)9 * i;
  bool ok = finite(a[0]) && finite(a[1]) && finite(a[2]);
  if (kind <= 1u) {
    ok = ok && finite(a[6]);
    if (kind == 1u)
      ok = ok && finite(a[3]) && finite(a[4]) && finite(a[5]) && finite(a[7]) && finite(a[8]) && a[8] > a[7];
  } else if (kind == 5u) {  // finite vertices and a non-zero, finite area (rtw_tri.hpp)
    double n[3], h;
    ok = ok && finite(a[3]) && finite(a[4]) && finite(a[5]) && finite(a[6]) && finite(a[7]) && finite(a[8]) &&
         rtwtri::derive(a, n, h);
  } else {
    ok = ok && finite(a[3]) && finite(a[4]);
  }
  if (!ok) {
    p.bad = p.bad + 1.0, p.first_bad = dmin(p.first_bad, (double)i);
    return;
  }
  double lo[3], hi[3];
  box_of(V, meta0, i, lo, hi);
  p.lo[0] = tmin(p.lo[0], lo[0]), p.lo[1] = tmin(p.lo[1], lo[1]), p.lo[2] = tmin(p.lo[2], lo[2]);
  p.hi[0] = tmax(p.hi[0], hi[0]), p.hi[1] = tmax(p.hi[1], hi[1]), p.hi[2] = tmax(p.hi[2], hi[2]);
  const uint32_t m = V.mate[i];
  if (m == kNone || !eligible(meta0, a)) return;
  if (m != i && !eligible(prim_meta0(V, V.order[m]), V.a + (size_t)9 * m)) return;
  double r[11];
  fill_record(kind, a, r);
  p.cc = dmax(p.cc, dmax(__builtin_fabs(r[0]), dmax(__builtin_fabs(r[1]), __builtin_fabs(r[2]))));
  p.cd = dmax(p.cd, dmax(__builtin_fabs(r[3]), dmax(__builtin_fabs(r[4]), __builtin_fabs(r[5]))));
  p.rho = dmax(p.rho, 2.0 * r[9] + 1.0);
}
RTWR_HD void validate_xform(const View& V, uint32_t xi, Partial& p) {
  if (!V.xv) return;
  const uint32_t h = ld_u32(V.xform + (size_t)rtwk::kWorldRec * xi, 0);
  const double* v = V.xv + (size_t)3 * rtwk::kMaxXfOps * xi;
  bool ok = true;
  for (uint32_t k = 0; k < rtwk::kMaxXfOps; ++k)
    if (k < xform_ops(h)) ok = ok && finite(v[3 * k]) && finite(v[3 * k + 1]) && finite(v[3 * k + 2]);
  if (!ok) p.bad = p.bad + 1.0, p.first_bad = dmin(p.first_bad, (double)V.n_prims + (double)xi);
}

// Commit, list index i: doubles 0-10 of its record (the meta doubles stay).
RTWR_HD void commit_prim(const View& V, uint32_t i) {
  const uint32_t pos = V.order[i];
  double* d = V.prim + (size_t)rtwk::kWorldRec * pos;
  if ((prim_meta0(V, pos) & 0xFFu) == 5u) {  // a triangle: doubles 0-10, 12, 13
    double t[14];
    (void)fill_record_tri(V.a + (size_t)9 * i, t);
    for (int k = 0; k < 11; ++k) d[k] = t[k];
    d[12] = t[12], d[13] = t[13];
    return;
  }
  double r[11];
  fill_record(prim_meta0(V, pos) & 0xFFu, V.a + (size_t)9 * i, r);
  for (int k = 0; k < 11; ++k) d[k] = r[k];
  // (a rebuild can move a triangle's record out of this position: no stale n.z, h behind it.  Worlds without
  // triangles hold zeros there and write nothing more than before.)
  if (V.has_tri) d[12] = 0.0, d[13] = 0.0;
}
RTWR_HD void commit_xform(const View& V, uint32_t xi) {
  if (!V.xv) return;
  double* d = V.xform + (size_t)rtwk::kWorldRec * xi;
  const uint32_t n = xform_ops(ld_u32(d, 0));
  const double* v = V.xv + (size_t)3 * rtwk::kMaxXfOps * xi;
  for (uint32_t k = 0; k < rtwk::kMaxXfOps; ++k)
    if (k < n) d[4 + 3 * k] = v[3 * k], d[5 + 3 * k] = v[3 * k + 1], d[6 + 3 * k] = v[3 * k + 2];
}

// Commit, node n: both child boxes (a leaf child from the INPUT numbers of its
// primitives, rounded outward; an interior child as the exact f32 union of
// that child's two boxes in the plain table, which a lower height wrote), the
// plain bounds, the node record's bounds (the ref's bytes re-embedded when the
// tree is packed) and refs (kCullBit by the rule of rtw_hip.h), and the
// pretest records of its candidate leaves.
RTWR_HD void commit_node(const View& V, uint32_t n) {
  float* nd = V.node + (size_t)rtwk::kNodeWords * n;
  float* pl = V.plain + (size_t)12 * n;
  const uint32_t cand = V.cand[n];
  for (int c = 0; c < 2; ++c) {
    const uint32_t ref0 = ld_u32(nd, 12 + c);
    const uint32_t ref = (ref0 & rtwk::kLeafBit) ? ref0 & ~rtwk::kCullBit : ref0;
    float l0, l1, l2, h0, h1, h2;
    uint32_t out_ref = ref;
    if (ref & rtwk::kLeafBit) {
      const uint32_t first = ref & 0x7FFFFFu, cnt = (ref >> 23) & rtwk::kLeafCountMask;
      double lo[3] = {inf(), inf(), inf()}, hi[3] = {-inf(), -inf(), -inf()};
      const bool is_cand = ((cand >> c) & 1u) != 0u;
      bool all = is_cand;
      for (uint32_t pos = first; pos < first + cnt; ++pos) {
        const uint32_t meta0 = prim_meta0(V, pos), li = prim_list_index(V, pos);
        double bl[3], bh[3];
        box_of(V, meta0, li, bl, bh);
        lo[0] = dmin(lo[0], bl[0]), lo[1] = dmin(lo[1], bl[1]), lo[2] = dmin(lo[2], bl[2]);
        hi[0] = dmax(hi[0], bh[0]), hi[1] = dmax(hi[1], bh[1]), hi[2] = dmax(hi[2], bh[2]);
        if (is_cand) {
          const double* a = V.a + (size_t)9 * li;
          all = all && eligible(meta0, a);
          if (V.has_table) {  // (every candidate leaf's record follows the numbers, so the table is a function of them)
            double r[11];
            fill_record(meta0 & 0xFFu, a, r);
            fill_cull(V.cull + (size_t)16 * first, pos - first, r);
          }
        }
      }
      if (all && V.has_table && V.cull_on) out_ref |= rtwk::kCullBit;
      l0 = down(lo[0]), l1 = down(lo[1]), l2 = down(lo[2]);
      h0 = up(hi[0]), h1 = up(hi[1]), h2 = up(hi[2]);
    } else {
      const float* q = V.plain + (size_t)12 * ref;
      l0 = fmin32(q[0], q[1]), l1 = fmin32(q[2], q[3]), l2 = fmin32(q[4], q[5]);
      h0 = fmax32(q[6], q[7]), h1 = fmax32(q[8], q[9]), h2 = fmax32(q[10], q[11]);
    }
    pl[0 + c] = l0, pl[2 + c] = l1, pl[4 + c] = l2, pl[6 + c] = h0, pl[8 + c] = h1, pl[10 + c] = h2;
    if (V.packed) {
      const uint32_t v = compact_ref(ref);
      l0 = lower_with_low8(l0, v & 255u), l1 = lower_with_low8(l1, (v >> 8) & 255u), l2 = lower_with_low8(l2, (v >> 16) & 255u);
    }
    nd[0 + c] = l0, nd[2 + c] = l1, nd[4 + c] = l2, nd[6 + c] = h0, nd[8 + c] = h1, nd[10 + c] = h2;
    st_u32(nd, 12 + c, out_ref);
  }
}

}  // namespace rtwr
