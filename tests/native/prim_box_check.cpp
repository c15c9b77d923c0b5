// prim_box (csrc/rtw_world_box.hpp) is conservative: the box the BVH builder
// (csrc/rtw_world_pack.cpp) gets for a primitive holds every point of the
// primitive, at every shutter time in [0, 1], after its Translate / RotateY chain.
//
// Random primitives of every kind (spheres, one radius in ten negative; moving
// spheres with their own time ranges, so the box is an extrapolation to times
// 0 and 1; the three rects) with chains of 0-4 ops.  Points on each surface
// are carried to world space in long double by a restatement of the
// reference's forward transforms (hittable.zig Translate.hit :487, RotateY.hit
// :583-585: op 0 is the outermost wrapper, so the innermost op applies first)
// that shares no code with the product.  Rects are sampled on their plane and
// on both faces of the reference's 1e-4 padding (hittable.zig:304-317).
//
// Slack: 1e-12 * (1 + max |coordinate| of the world point) — ~1e3 x the f64
// rounding of the few operations involved, ~1e5 x below the traversal's own
// margin (rtw_world_capi.hip bvh_margin: 1e-7 L).
//
// usage: prim_box_check N seed   ->  "violations V/POINTS", exit 1 if V > 0
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "rtw_world_box.hpp"

namespace {

typedef long double ld;

uint64_t g_s;
uint64_t next_u64() {  // splitmix64
  uint64_t z = (g_s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double uni() { return (double)(next_u64() >> 11) * 0x1p-53; }  // [0, 1)
double range(double a, double b) { return a + (b - a) * uni(); }
uint32_t below(uint32_t n) { return (uint32_t)(next_u64() % n); }

// The world-space point of an object-space point: the chain's wrappers from
// the innermost (op n-1) out to op 0.
void forward(const rtw_xform& xf, ld p[3]) {
  for (int i = (int)xf.n - 1; i >= 0; --i) {
    if (xf.op[i] == RTW_XF_TRANSLATE) {
      for (int k = 0; k < 3; ++k) p[k] += (ld)xf.v[i][k];
    } else {
      const ld sn = xf.v[i][0], cs = xf.v[i][1];
      const ld x = cs * p[0] + sn * p[2], z = -sn * p[0] + cs * p[2];
      p[0] = x, p[2] = z;
    }
  }
}

rtw_xform random_chain() {
  rtw_xform xf{};
  xf.n = below(RTW_MAX_XFORM_OPS + 1);
  for (uint32_t i = 0; i < xf.n; ++i) {
    xf.op[i] = below(2) ? RTW_XF_ROTATE_Y : RTW_XF_TRANSLATE;
    if (xf.op[i] == RTW_XF_TRANSLATE) {
      for (int k = 0; k < 3; ++k) xf.v[i][k] = range(-50, 50);
    } else {
      const double t = range(-3.2, 3.2);
      xf.v[i][0] = std::sin(t), xf.v[i][1] = std::cos(t), xf.v[i][2] = t;
    }
  }
  // one chain in eight: two adjacent translations of magnitude >= 1e3 that nearly cancel
  if (xf.n >= 2 && below(8) == 0) {
    const uint32_t i = below(xf.n - 1);
    xf.op[i] = xf.op[i + 1] = RTW_XF_TRANSLATE;
    for (int k = 0; k < 3; ++k) {
      const double big = (below(2) ? 1.0 : -1.0) * range(1000, 3000);
      xf.v[i][k] = big, xf.v[i + 1][k] = -big + range(-2, 2);
    }
  }
  return xf;
}

}  // namespace

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 100000;
  g_s = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  const int kPoints = 12;
  long points = 0, viol = 0, kinds[5] = {0, 0, 0, 0, 0}, chained[RTW_MAX_XFORM_OPS + 1] = {0};
  long double worst = 0;
  for (long it = 0; it < n; ++it) {
    rtw_prim p{};
    p.kind = below(5);
    kinds[p.kind]++;
    const rtw_xform xf = random_chain();
    p.xform = xf.n ? 0 : -1;
    chained[xf.n]++;
    if (p.kind <= RTW_PRIM_MOVING_SPHERE) {
      for (int k = 0; k < 3; ++k) p.a[k] = p.a[3 + k] = range(-20, 20);
      double r = below(4) == 0 ? range(50, 1000) : range(0.05, 5);
      if (below(10) == 0) r = -r;
      p.a[6] = r;
      if (p.kind == RTW_PRIM_MOVING_SPHERE) {
        for (int k = 0; k < 3; ++k) p.a[3 + k] = p.a[k] + range(-3, 3);
        if (below(3) == 0) {
          p.a[7] = 0.0, p.a[8] = 1.0;
        } else {  // its own range: inside, around or beside the shutter [0, 1]
          p.a[7] = range(-2, 1);
          p.a[8] = p.a[7] + range(0.1, 3);
        }
      }
    } else {
      p.a[0] = range(-20, 20), p.a[1] = p.a[0] + range(0.01, 30);
      p.a[2] = range(-20, 20), p.a[3] = p.a[2] + range(0.01, 30);
      p.a[4] = range(-20, 20);
    }
    const Box b = prim_box(p, xf.n ? &xf : nullptr);
    for (int s = 0; s < kPoints; ++s) {
      ld q[3];
      if (p.kind <= RTW_PRIM_MOVING_SPHERE) {
        ld d[3], len = 0;
        do {
          len = 0;
          for (int k = 0; k < 3; ++k) d[k] = (ld)range(-1, 1), len += d[k] * d[k];
        } while (len > 1 || len < 1e-6L);
        len = sqrtl(len);
        if (s < 6) {  // the six axis extremes: the points that touch the box of an unrotated sphere
          for (int k = 0; k < 3; ++k) d[k] = 0;
          d[s / 2] = (s & 1) ? 1 : -1;
          len = 1;
        }
        // shutter times: both ends and inside
        const ld t = s % 3 == 0 ? 0.0L : (s % 3 == 1 ? 1.0L : (ld)uni());
        const ld r = fabsl((ld)p.a[6]);
        for (int k = 0; k < 3; ++k) {
          ld c = p.a[k];
          if (p.kind == RTW_PRIM_MOVING_SPHERE)  // MovingSphere.center, hittable.zig:219-221
            c = (ld)p.a[k] + ((ld)p.a[3 + k] - (ld)p.a[k]) * ((t - (ld)p.a[7]) / ((ld)p.a[8] - (ld)p.a[7]));
          q[k] = c + r * d[k] / len;
        }
      } else {
        const int ax_k = p.kind == RTW_PRIM_XY_RECT ? 2 : (p.kind == RTW_PRIM_XZ_RECT ? 1 : 0);
        const int ax_a = p.kind == RTW_PRIM_YZ_RECT ? 1 : 0, ax_b = p.kind == RTW_PRIM_XY_RECT ? 1 : 2;
        // the four corners, then interior points
        const ld u = s < 4 ? (ld)(s & 1) : (ld)uni(), v = s < 4 ? (ld)(s >> 1) : (ld)uni();
        q[ax_a] = (ld)p.a[0] + u * ((ld)p.a[1] - (ld)p.a[0]);
        q[ax_b] = (ld)p.a[2] + v * ((ld)p.a[3] - (ld)p.a[2]);
        // on the plane, and on both faces of the reference's padding
        const ld pad = (ld)0.0001;
        q[ax_k] = (ld)p.a[4] + (s % 3 == 0 ? 0.0L : (s % 3 == 1 ? pad : -pad));
      }
      if (xf.n) forward(xf, q);
      ld m = 0;
      for (int k = 0; k < 3; ++k) m = std::max(m, fabsl(q[k]));
      const ld slack = 1e-12L * (1 + m);
      bool bad = false;
      for (int k = 0; k < 3; ++k) {
        const ld out = std::max((ld)b.lo[k] - q[k], q[k] - (ld)b.hi[k]);
        worst = std::max(worst, out / (1 + m));
        bad = bad || !(out <= slack);
      }
      ++points;
      if (bad && viol++ < 5)
        fprintf(stderr, "prim kind %u chain %u: (%.17Lg %.17Lg %.17Lg) outside [%.17g %.17g] [%.17g %.17g] [%.17g %.17g]\n",
                p.kind, xf.n, q[0], q[1], q[2], b.lo[0], b.hi[0], b.lo[1], b.hi[1], b.lo[2], b.hi[2]);
    }
  }
  printf("prims %ld (kinds %ld %ld %ld %ld %ld; chains of 0-4 ops %ld %ld %ld %ld %ld) worst excess %.3Lg x (1 + max|coord|)\n",
         n, kinds[0], kinds[1], kinds[2], kinds[3], kinds[4], chained[0], chained[1], chained[2], chained[3], chained[4],
         worst);
  printf("violations %ld/%ld\n", viol, points);
  return viol ? 1 : 0;
}
