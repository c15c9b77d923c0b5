// rtw_world_box.hpp — world-space bounding boxes of the general world's
// primitives (the BVH builder's input, rtw_world_pack.cpp).  Host only, no
// HIP: tests/native/prim_box_check.cpp compiles it with a plain C++ compiler
// and checks that every box holds its primitive.
#pragma once

#include <algorithm>
#include <cmath>

#include "rtw_hip.h"

namespace {

struct Box {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  void grow(const Box& b) {
    for (int k = 0; k < 3; ++k) lo[k] = std::min(lo[k], b.lo[k]), hi[k] = std::max(hi[k], b.hi[k]);
  }
  void grow(const double p[3]) {
    for (int k = 0; k < 3; ++k) lo[k] = std::min(lo[k], p[k]), hi[k] = std::max(hi[k], p[k]);
  }
  double area() const {
    const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return dx < 0 ? 0.0 : 2.0 * (dx * dy + dy * dz + dz * dx);
  }
};

// World-space bounding box of a primitive: the reference's boudingBox
// (hittable.zig:133-143 sphere, :203-217 moving sphere over the camera
// shutter [0, 1], :304-317 / :359-372 / :414-427 rects padded by 1e-4)
// through its Translate / RotateY chain (:493-501, :514-556).
Box prim_box(const rtw_prim& p, const rtw_xform* xf) {
  Box b;
  if (p.kind <= RTW_PRIM_MOVING_SPHERE) {
    const double r = std::fabs(p.a[6]);
    for (int s = 0; s < (p.kind == RTW_PRIM_MOVING_SPHERE ? 2 : 1); ++s) {
      double c[3];
      for (int k = 0; k < 3; ++k) {
        c[k] = p.kind == RTW_PRIM_MOVING_SPHERE ? p.a[k] + (p.a[3 + k] - p.a[k]) * (((double)s - p.a[7]) / (p.a[8] - p.a[7]))
                                                : p.a[k];
      }
      Box cb;
      for (int k = 0; k < 3; ++k) cb.lo[k] = c[k] - r, cb.hi[k] = c[k] + r;
      b.grow(cb);
    }
  } else if (p.kind == RTW_PRIM_TRIANGLE) {  // its vertices' box, padded by 1e-4 on every axis
    for (int k = 0; k < 3; ++k) {
      b.lo[k] = std::min(std::min(p.a[k], p.a[3 + k]), p.a[6 + k]) - 0.0001;
      b.hi[k] = std::max(std::max(p.a[k], p.a[3 + k]), p.a[6 + k]) + 0.0001;
    }
  } else {
    const int ax_k = p.kind == RTW_PRIM_XY_RECT ? 2 : (p.kind == RTW_PRIM_XZ_RECT ? 1 : 0);
    const int ax_a = p.kind == RTW_PRIM_YZ_RECT ? 1 : 0, ax_b = p.kind == RTW_PRIM_XY_RECT ? 1 : 2;
    b.lo[ax_a] = p.a[0], b.hi[ax_a] = p.a[1];
    b.lo[ax_b] = p.a[2], b.hi[ax_b] = p.a[3];
    b.lo[ax_k] = p.a[4] - 0.0001, b.hi[ax_k] = p.a[4] + 0.0001;
  }
  if (xf) {
    for (int i = (int)xf->n - 1; i >= 0; --i) {
      if (xf->op[i] == RTW_XF_TRANSLATE) {
        for (int k = 0; k < 3; ++k) b.lo[k] += xf->v[i][k], b.hi[k] += xf->v[i][k];
      } else {
        const double sn = xf->v[i][0], cs = xf->v[i][1];
        Box nb;
        for (int c = 0; c < 8; ++c) {
          const double x = (c & 1) ? b.hi[0] : b.lo[0], y = (c & 2) ? b.hi[1] : b.lo[1],
                       z = (c & 4) ? b.hi[2] : b.lo[2];
          const double q[3] = {cs * x + sn * z, y, -sn * x + cs * z};
          nb.grow(q);
        }
        b = nb;
      }
    }
  }
  return b;
}

}  // namespace
