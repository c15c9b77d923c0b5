// rtw_world_tex.hpp — Texture.value over the world's device tables, shared by
// the render kernel (rtw_world.hip: the shade and the feature buffers) and the
// surface queries (rtw_surface.hip).  One text, so the value a caller reads at a
// hit is the value the render multiplies in, bit for bit.  Device code.
//
// Indices: `ti`, the texture's perlin and image fields were checked against
// their tables when the world was packed (rtw_world_pack.cpp).  What depends on
// u, v and p — the caller's numbers in a surface query — is masked (the Perlin
// lattice, & 255 of a saturating conversion) or clamped (the image's column and
// row) before it indexes anything, so no value of u, v, p leaves the tables.
#pragma once
#include "rtw_libm.hpp"
#include "rtw_world_walk.hpp"

namespace rtwk {

// Texture.value (texture.zig:36-144) for the winner's record.
template <int FEAT, typename WV>
__device__ __forceinline__ V tex_value(const WV& W, uint32_t ti, D u, D v, V p) {
  const D* t = W.tex + kWorldRec * ti;
  const uint32_t* th = reinterpret_cast<const uint32_t*>(t);
  switch (th[0]) {
    case 1u:  // checker: only the sign of sin(10x) sin(10y) sin(10z) matters (rtw_math.hpp)
      return rtwm::checker_odd((D)10 * p.x, (D)10 * p.y, (D)10 * p.z) ? ld3(t + 5) : ld3(t + 8);
    case 2u: {  // noise
      if constexpr (!(FEAT & kFeatNoise)) return mk(0.0, 0.0, 0.0);  // (no noise texture in this world), texture.zig:101-105 + Perlin.turb/noise (perlin.zig:49-91)
      const D* pr = W.perlin + (size_t)th[1] * (256 * 3 + 384);
      const uint32_t* perm = reinterpret_cast<const uint32_t*>(pr + 256 * 3);
      D accum = 0.0, weight = 1.0;
      V q = p;
      // Rolled loops (one corner at a time): unrolled, the 56 corner
      // evaluations would set the whole kernel's register budget.
#pragma unroll 1
      for (int oct = 0; oct < 7; ++oct) {
        const D fx = floor(q.x), fy = floor(q.y), fz = floor(q.z);
        const D uu0 = q.x - fx, vv0 = q.y - fy, ww0 = q.z - fz;
        const D uu = uu0 * uu0 * (3 - 2 * uu0), vv = vv0 * vv0 * (3 - 2 * vv0), ww = ww0 * ww0 * (3 - 2 * ww0);
        const int i = (int)fx, j = (int)fy, k = (int)fz;
        D nz = 0.0;
#pragma unroll 1
        for (int cr = 0; cr < 8; ++cr) {  // perlinInterp's i, j, k loops (perlin.zig:104-124), in order
          const int di = cr >> 2, dj = (cr >> 1) & 1, dk = cr & 1;
          const uint32_t ix = (uint32_t)(i + di) & 255u, iy = (uint32_t)(j + dj) & 255u, iz = (uint32_t)(k + dk) & 255u;
          const D* c = pr + 3 * (perm[ix] ^ perm[256 + iy] ^ perm[512 + iz]);
          const D ti = (D)di, tj = (D)dj, tk = (D)dk;
          const V wgt = mk(uu - ti, vv - tj, ww - tk);
          nz += (ti * uu + (1.0 - ti) * (1.0 - uu)) * (tj * vv + (1.0 - tj) * (1.0 - vv)) *
                (tk * ww + (1.0 - tk) * (1.0 - ww)) * dot(ld3(c), wgt);
        }
        accum += weight * nz;
        weight *= 0.5;
        q = mk(q.x * 2.0, q.y * 2.0, q.z * 2.0);
      }
      const D kk = 0.5 * (1.0 + rtwl::sin(t[11] * p.z + 10.0 * fabs(accum)));
      return mk(1 * kk, 1 * kk, 1 * kk);
    }
    case 3u: {  // image
      if constexpr (!(FEAT & kFeatImage)) return mk(0.0, 0.0, 0.0);  // (no image texture in this world), texture.zig:121-144 (row clamp: rtw_world.h)
      const uint32_t* im = W.image + 4 * th[2];
      const uint32_t w = im[0], hgt = im[1];
      const D uc = fmax(0.0, fmin(u, 1.0));
      const D vc = 1.0 - fmax(0.0, fmin(v, 1.0));
      const uint64_t i = (uint64_t)(uc * (D)w), j = (uint64_t)(vc * (D)hgt);
      const uint64_t i_ = i < w - 1 ? i : w - 1;
      uint64_t j_ = j < w - 1 ? j : w - 1;
      if (j_ > hgt - 1) j_ = hgt - 1;
      const uint8_t* px = W.pixels + ((uint64_t)im[2] | ((uint64_t)im[3] << 32)) + (j_ * w + i_) * 4;
      const uchar4 c = *reinterpret_cast<const uchar4*>(px);
      if (c.w == 0) return mk(0.0, 0.0, 1.0);
      const D s = 1.0 / 255.0;
      return mk(s * (D)c.x, s * (D)c.y, s * (D)c.z);
    }
    default:
      return ld3(t + 2);
  }
}

}  // namespace rtwk
