// rtw_surface.hip — surface queries (rtw_hip.h "surface queries", DESIGN.md
// §19): for each hit record of a ray query, what the hit surface IS — the
// material's kind and index, its texture's value at the record's u, v, p (the
// render's own tex_value, rtw_world_tex.hpp), a metal's fuzz, a glass's index —
// and, from the same numbers, the rtw_guide record the feature-buffer kernels
// would have written for that ray.
//
// One lane per record, 256 per workgroup, one launch.  The 80-byte hit record
// is read with 8-byte loads (its alignment), the tables (order, primitive meta,
// material, texture, Perlin, image) are per-lane gathers that stay in cache, the
// surface record leaves as eight 8-byte words and the guide as guide_store
// writes it (two 16-byte stores).  No LDS, no atomics, no workspace.  The hit
// records are the caller's memory: `prim` is checked against the list here
// (prev_points_kernel's rule), and everything u, v, p index is masked or clamped
// in tex_value; every other index is a table's own, checked when it was packed.
// -ffp-contract=off (Makefile).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "rtw_capi_shared.hpp"
#include "rtw_denoise.hpp"  // rtwd::Guide = rtw_guide
#include "rtw_surface.hpp"
#include "rtw_world_tex.hpp"

namespace rtwk {

namespace {

struct WorldSurfaceArgs {
  WorldView w;
  const double* hits;  // n x rtw_hit (10 x 8 bytes)
  uint64_t* surf;      // n x rtw_surface (8 x 8 bytes), or null
  rtwd::Guide* guides; // n x rtw_guide, or null
  double bg[3];        // a miss's albedo (read only with guides)
  uint32_t n;          // <= 2^31
};
struct SceneSurfaceArgs {
  SceneView<double> sc;
  const double* hits;
  uint64_t* surf;
  rtwd::Guide* guides;
  double bg[3];
  uint32_t n;
};

// What a lane found out about its record; by value, in registers.
struct Surf {
  V value;
  D fuzz, ir;
  uint32_t kind, mat, tex, tex_kind;  // each + 1; 0: none
};

__device__ __forceinline__ uint64_t bits(D x) { return __builtin_bit_cast(uint64_t, x); }

// The two stores of a record.  A miss (s: all zero, +0.0): 64 zero bytes; {0, 0, 0, 0, f32(background), 0}.
__device__ __forceinline__ void surface_store(uint64_t* surf, rtwd::Guide* guides, uint32_t i, bool hit, const Surf s,
                                              const double* h, uint32_t prim, const double* bg) {
  if (surf) {  // (uniform)
    uint64_t* o = surf + (size_t)8 * i;
    o[0] = bits(s.value.x), o[1] = bits(s.value.y), o[2] = bits(s.value.z);
    o[3] = bits(s.fuzz), o[4] = bits(s.ir);
    o[5] = (uint64_t)s.kind | ((uint64_t)s.mat << 32);
    o[6] = (uint64_t)s.tex | ((uint64_t)s.tex_kind << 32);
    o[7] = 0ull;  // reserved
  }
  if (guides) {  // (uniform)
    rtwd::Guide g;
    if (hit) {
      g.n[0] = (float)h[4], g.n[1] = (float)h[5], g.n[2] = (float)h[6];
      g.depth = (float)h[0];
      g.albedo[0] = (float)s.value.x, g.albedo[1] = (float)s.value.y, g.albedo[2] = (float)s.value.z;
      g.prim = prim;
    } else {
      g.n[0] = 0.0f, g.n[1] = 0.0f, g.n[2] = 0.0f;
      g.depth = 0.0f;
      g.albedo[0] = (float)bg[0], g.albedo[1] = (float)bg[1], g.albedo[2] = (float)bg[2];
      g.prim = 0u;
    }
    guides[i] = g;
  }
}

// FEAT: the world's feature set (rtw_world.hip world_feature_set): a world
// without noise or image textures does not carry their registers.
template <int FEAT>
__global__ void __launch_bounds__(256) world_surface_kernel(WorldSurfaceArgs A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;  // (n <= 2^31)
  if (i >= A.n) return;
  const WorldView& W = A.w;
  const double* h = A.hits + (size_t)10 * i;
  const uint32_t prim = (uint32_t)reinterpret_cast<const uint64_t*>(h)[9];
  const bool hit = prim != 0u && prim <= W.n_prims;
  Surf s;
  s.value = mk(0.0, 0.0, 0.0), s.fuzz = 0.0, s.ir = 0.0;
  s.kind = 0u, s.mat = 0u, s.tex = 0u, s.tex_kind = 0u;
  if (hit) {
    const uint32_t* mt = meta_of(W.prim + (size_t)kWorldRec * W.order[prim - 1u]);
    const D* mp = W.mat + (size_t)8 * mt[1];
    const uint32_t* mh = reinterpret_cast<const uint32_t*>(mp);
    const uint32_t mkind = mh[0], mtex = mh[1];
    s.kind = mkind + 1u, s.mat = mt[1] + 1u;
    if (mkind == 1u) {  // metal
      s.value = ld3(mp + 1);
      s.fuzz = mp[4];
    } else if (mkind == 2u) {  // dielectric
      s.value = mk(1.0, 1.0, 1.0);
      s.ir = mp[5];
    } else {  // Lambert's albedo texture, a light's emit texture
      s.value = tex_value<FEAT>(W, mtex, h[7], h[8], mk(h[1], h[2], h[3]));
      s.tex = mtex + 1u;
      s.tex_kind = *reinterpret_cast<const uint32_t*>(W.tex + (size_t)kWorldRec * mtex) + 1u;
    }
  }
  surface_store(A.surf, A.guides, i, hit, s, h, prim, A.bg);
}

// The cover scene's table (rtw_internal.hpp "HBM layout of a scene"), reported in
// the world's enumerations: rtw_material_kind 0, 1 are Lambert over a solid and a
// checker texture; there is no texture table (tex = 0).
__global__ void __launch_bounds__(256) scene_surface_kernel(SceneSurfaceArgs A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= A.n) return;
  const SceneView<double>& S = A.sc;
  const double* h = A.hits + (size_t)10 * i;
  const uint32_t prim = (uint32_t)reinterpret_cast<const uint64_t*>(h)[9];
  const bool hit = prim != 0u && prim <= S.n;
  Surf s;
  s.value = mk(0.0, 0.0, 0.0), s.fuzz = 0.0, s.ir = 0.0;
  s.kind = 0u, s.mat = 0u, s.tex = 0u, s.tex_kind = 0u;
  if (hit) {
    const uint32_t mi = (S.meta[S.perm[prim - 1u]] >> 8) & 0xFFFu;
    const D* mp = S.mat + (size_t)8 * mi;
    const uint32_t kind = S.kind[mi];
    s.mat = mi + 1u;
    s.value = ld3(mp);  // solid colour, checker even colour, metal albedo
    if (kind <= 1u) {
      s.kind = 1u, s.tex_kind = kind + 1u;
      if (kind == 1u && rtwm::checker_odd(10.0 * h[1], 10.0 * h[2], 10.0 * h[3])) s.value = ld3(mp + 3);
    } else if (kind == 2u) {
      s.kind = 2u, s.fuzz = mp[6];
    } else {
      s.kind = 3u, s.value = mk(1.0, 1.0, 1.0), s.ir = mp[7];
    }
  }
  surface_store(A.surf, A.guides, i, hit, s, h, prim, A.bg);
}

template <int FEAT>
void launch_world_surface_feat(const WorldSurfaceArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(world_surface_kernel<FEAT>, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a);
}

}  // namespace

}  // namespace rtwk

namespace {

int surface_args(const char* who, const rtw_hit* d_hits, uint64_t n, const double* bg, rtw_surface* d_surf,
                 rtw_guide* d_guides, bool* launch) {
  std::string msg;
  const int st = rtws::check_call(who, d_hits, n, bg, d_surf, d_guides, launch, msg);
  return st == RTW_OK ? RTW_OK : rtw_fail(st, "%s", msg.c_str());
}

template <typename Args>
void fill_common(Args& a, const rtw_hit* d_hits, uint64_t n, const double* bg, rtw_surface* d_surf, rtw_guide* d_guides) {
  a.hits = reinterpret_cast<const double*>(d_hits);
  a.surf = reinterpret_cast<uint64_t*>(d_surf);
  a.guides = reinterpret_cast<rtwd::Guide*>(d_guides);
  for (int k = 0; k < 3; ++k) a.bg[k] = (d_guides && bg) ? bg[k] : 0.0;
  a.n = (uint32_t)n;
}

}  // namespace

extern "C" {

int rtw_world_surface_device(rtw_world w, const rtw_hit* d_hits, uint64_t n, const double background[3],
                             rtw_surface* d_surf, rtw_guide* d_guides, void* stream) {
  using namespace rtwk;
  const char* who = "rtw_world_surface_device";
  WorldSurfaceArgs a;
  std::memset(&a, 0, sizeof(a));
  uint32_t feat = 0;
  int st = rtw_world_view(w, who, &a.w, &feat);  // (NULL, or a world of another device: RTW_EINVAL)
  if (st != RTW_OK) return st;
  bool launch = false;
  st = surface_args(who, d_hits, n, background, d_surf, d_guides, &launch);
  if (st != RTW_OK || !launch) return st;
  fill_common(a, d_hits, n, background, d_surf, d_guides);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int fs = world_feature_set(feat, false, false);
  if (fs == (kFeatImage | kFeatTri))
    launch_world_surface_feat<kFeatImage | kFeatTri>(a, s);
  else if (fs == (kFeatAll | kFeatTri))
    launch_world_surface_feat<kFeatAll | kFeatTri>(a, s);
  else if (fs == kFeatImage)
    launch_world_surface_feat<kFeatImage>(a, s);
  else if (fs == (kFeatXform | kFeatRect))
    launch_world_surface_feat<kFeatXform | kFeatRect>(a, s);
  else
    launch_world_surface_feat<kFeatAll>(a, s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "%s: kernel launch: %s", who, hipGetErrorString(e));
  return RTW_OK;
}

int rtw_scene_surface_device(rtw_scene sc, const rtw_hit* d_hits, uint64_t n, const double background[3],
                             rtw_surface* d_surf, rtw_guide* d_guides, void* stream) {
  using namespace rtwk;
  const char* who = "rtw_scene_surface_device";
  SceneSurfaceArgs a;
  std::memset(&a, 0, sizeof(a));
  int st = rtw_scene_view(sc, who, &a.sc);
  if (st != RTW_OK) return st;
  bool launch = false;
  st = surface_args(who, d_hits, n, background, d_surf, d_guides, &launch);
  if (st != RTW_OK || !launch) return st;
  fill_common(a, d_hits, n, background, d_surf, d_guides);
  hipLaunchKernelGGL(scene_surface_kernel, dim3((a.n + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return rtw_fail(RTW_EHIP, "%s: kernel launch: %s", who, hipGetErrorString(e));
  return RTW_OK;
}

int rtw_world_surface(rtw_world w, const rtw_hit* hits, uint64_t n, rtw_surface* surf_out) {
  const char* who = "rtw_world_surface";
  if (!w) return rtw_fail(RTW_EINVAL, "%s: world is NULL", who);
  if (n > RTW_QUERY_MAX_RAYS) return rtw_fail(RTW_EINVAL, "%s: n > 2^31", who);
  if (n == 0) return RTW_OK;
  if (!hits || !surf_out) return rtw_fail(RTW_EINVAL, "%s: hits or surf_out is NULL", who);
  struct Bufs {  // freed on every way out
    rtw_hit* h = nullptr;
    rtw_surface* s = nullptr;
    ~Bufs() {
      if (h) (void)hipFree(h);
      if (s) (void)hipFree(s);
    }
  } b;
  if (hipMalloc(reinterpret_cast<void**>(&b.h), n * sizeof(rtw_hit)) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&b.s), n * sizeof(rtw_surface)) != hipSuccess)
    return rtw_fail(RTW_ENOMEM, "%s: device buffers for %llu records", who, (unsigned long long)n);
  if (hipMemcpy(b.h, hits, n * sizeof(rtw_hit), hipMemcpyHostToDevice) != hipSuccess)
    return rtw_fail(RTW_EHIP, "%s: copy of the records failed", who);
  const int st = rtw_world_surface_device(w, b.h, n, nullptr, b.s, nullptr, nullptr);
  if (st != RTW_OK) return st;
  if (hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(surf_out, b.s, n * sizeof(rtw_surface), hipMemcpyDeviceToHost) != hipSuccess)
    return rtw_fail(RTW_EHIP, "%s: the query failed on the device", who);
  return RTW_OK;
}

}  // extern "C"
