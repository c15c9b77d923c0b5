// rtw_query.hip — ray queries (rtw_hip.h "ray queries"): the
// closest hit, or the occlusion, of rays the caller supplies, over an uploaded
// world or scene.  The walks are the render's (rtw_world_walk.hpp): the linear
// loop and the wave's union walk with one ray per lane and a grid-stride over
// the batch, or the resumable per-lane walk with lane-level regeneration — a
// lane whose walk finished writes its record and takes the wave's next ray
// while the other lanes keep walking.  Each ray brings its own time, t_min and
// t_max (the initial closest).  f64, one IEEE operation per reference
// operation; every record equals the oracle's rw_hit bit for bit.
#include <hip/hip_runtime.h>

#include "rtw_device.hpp"
#include "rtw_libm.hpp"
#include "rtw_query_dev.hpp"
#include "rtw_scene_hit.hpp"
#include "rtw_world_walk.hpp"

namespace rtwk {

namespace {

// What a lane does with its finished walk: the NaN fallback, then the record
// (or the occlusion byte).
template <int FEAT, bool OCCL>
__device__ __forceinline__ void finish_ray(const WorldQueryArgs& A, const WorldView& W, uint64_t i, const QRay& q,
                                           WHit& h) {
  if (__builtin_expect(h.nan != 0u, 0)) {
    if (!OCCL || h.pos < 0) seq_hit<FEAT>(W, W.order, q.o, q.d, q.time, q.tmin, h, q.tmax);
  }
  if constexpr (OCCL) {
    static_cast<uint8_t*>(A.out)[i] = h.pos >= 0 ? (uint8_t)1 : (uint8_t)0;
  } else {
    if (h.pos < 0) {
      store_miss(A.out, i);
    } else {
      const HitRec R = hit_record<FEAT>(W, h.pos, h.t, q.o, q.d, q.time, true);
      store_hit(A.out, i, h.t, R, (uint32_t)h.orig + 1u);
    }
  }
}

// Linear loop / union walk: 64 rays per wave step, grid-stride over the batch.
template <int FEAT, bool OCCL>
__global__ void __launch_bounds__(kQueryBlock) world_query_kernel(WorldQueryArgs A) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  uint32_t* stack = reinterpret_cast<uint32_t*>(lds_raw) + (threadIdx.x >> 6) * kBvhStack;  // this wave's
  const WorldView& W = A.w;
  const uint32_t lid = lane_id();
  const uint64_t waves = (uint64_t)gridDim.x * (kQueryBlock / 64);
  unsigned long long nv = 0, nt = 0;
  KStats st;
  for (uint64_t base = ((uint64_t)blockIdx.x * (kQueryBlock / 64) + (threadIdx.x >> 6)) * 64u; base < A.n;
       base += waves * 64u) {  // (wave-uniform)
    const uint64_t i = base + lid;
    if (i < A.n) {
      const QRay q = load_ray(A.rays, i);
      WHit h;
      closest<0, FEAT, OCCL, true>(W, ray_margin(A.reach, q.o), stack, q.o, q.d, q.time, q.tmin, h, nv, nt, st, q.tmax);
      if (A.seq_times && (q.time < 0.0 || q.time > 1.0)) h.nan = 1u, h.pos = -1;
      finish_ray<FEAT, OCCL>(A, W, i, q, h);
    }
  }
}

// Per-lane walk (sphere worlds with a BVH): wave w takes the batch's 64-ray
// blocks w, w + waves, ...; its k-th ray is ray (k & 63) of block
// w + (k >> 6) * waves.  A lane without a walk takes the wave's next ray; the
// phase yields while rays remain, so finished lanes do not wait for the
// wave's longest walk.
template <int FEAT, bool OCCL>
__global__ void __launch_bounds__(kQueryBlock, 4) world_query_lane_kernel(WorldQueryArgs A) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  constexpr uint32_t kWaveWords = (kLaneStackLds + kTravWords) * 64u;
  uint32_t* stack = reinterpret_cast<uint32_t*>(lds_raw) + (threadIdx.x >> 6) * kWaveWords;
  LaneTravRows* rows = reinterpret_cast<LaneTravRows*>(stack + kLaneStackLds * 64u);
  const WorldView& W = A.w;
  const uint32_t lid = lane_id();
  constexpr bool NCACHE = (FEAT & kFeatPacked) != 0 && kNodeCache > 0;
  const nf4* node_cache = nullptr;
  if constexpr (NCACHE) {  // the top of the tree, as world_kernel stages it
    __shared__ nf4 ncache_lds[(kNodeCache > 0 ? kNodeCache : 1u) * 3u];
    const uint32_t nn = min(W.n_nodes, kNodeCache);
    const nf4* gn = reinterpret_cast<const nf4*>(W.node);
    for (uint32_t i = threadIdx.x; i < 3u * nn; i += kQueryBlock) ncache_lds[i] = gn[(i / 3u) * 4u + i % 3u];
    __syncthreads();
    node_cache = ncache_lds;
  }
  const uint64_t waves = (uint64_t)gridDim.x * (kQueryBlock / 64);
  const uint64_t wave = (uint64_t)blockIdx.x * (kQueryBlock / 64) + (threadIdx.x >> 6);
  auto ray_index = [&](uint32_t k) -> uint64_t { return ((wave + (uint64_t)(k >> 6) * waves) << 6) + (k & 63u); };
  uint32_t k = 0;  // (wave-uniform) rays of this wave handed out
  bool walking = false, done = false;
  uint64_t mine = 0;
  QRay q;
  q.o = mk(0.0, 0.0, 0.0), q.d = mk(1.0, 1.0, 1.0), q.time = 0.0, q.tmin = 0.0, q.tmax = 0.0;
  unsigned long long nv = 0, nt = 0, wi = 0, wl = 0;
  for (;;) {
    const bool need = !walking && !done;
    const uint64_t nm = wballot(need);
    if (nm) {
      if (need) {
        const uint64_t i = ray_index(k + mbcnt64(nm));
        if (i >= A.n) {
          done = true;  // (indices grow with k: so are this lane's later ones)
        } else {
          q = load_ray(A.rays, i);
          mine = i;
          trav_begin(rows, lid, q.tmax);
          walking = true;
        }
      }
      k += popc64(nm);
    }
    if (!wany(walking)) break;
    const uint32_t yl = ray_index(k) < A.n ? A.lane_yield : 0u;  // nothing to take: walk to the end
    WHit h;
    if (trav_phase<0, FEAT, OCCL, true>(W, ray_margin(A.reach, q.o), stack, rows, node_cache, lid, walking, yl, q.o, q.d, q.time,
                                  q.tmin, h, nv, nt, wi, wl)) {
      walking = false;
      if (A.seq_times && (q.time < 0.0 || q.time > 1.0)) h.nan = 1u, h.pos = -1;
      finish_ray<FEAT, OCCL>(A, W, mine, q, h);
    }
  }
}

// Scenes: scene_closest (rtw_scene_hit.hpp, shared with scene_guides_kernel) over
// the packed sphere table, with the ray's own time, t_min and t_max.
template <bool OCCL>
__global__ void __launch_bounds__(kQueryBlock) scene_query_kernel(SceneQueryArgs A) {
  const SceneView<D>& S = A.sc;
  const uint32_t lid = lane_id();
  const uint64_t waves = (uint64_t)gridDim.x * (kQueryBlock / 64);
  for (uint64_t base = ((uint64_t)blockIdx.x * (kQueryBlock / 64) + (threadIdx.x >> 6)) * 64u; base < A.n;
       base += waves * 64u) {
    const uint64_t i = base + lid;
    if (i >= A.n) continue;
    const QRay q = load_ray(A.rays, i);
    const V &o = q.o, &d = q.d;
    const SceneHit sh = scene_closest<OCCL>(S, o, d, q.time, q.tmin, q.tmax);
    const int hit = sh.pos, hit_orig = sh.orig;
    const D hit_t = sh.t;
    if constexpr (OCCL) {
      static_cast<uint8_t*>(A.out)[i] = hit >= 0 ? (uint8_t)1 : (uint8_t)0;
    } else {
      if (hit < 0) {
        store_miss(A.out, i);
        continue;
      }
      const uint32_t meta = S.meta[hit];
      HitRec R;
      R.p = add(o, mul(d, hit_t));
      const V c = scene_center(S, (uint32_t)hit, meta, q.time);
      const V outward = divs(sub(R.p, c), S.rad[hit]);
      R.front = dot(outward, d) < 0.0;
      R.nrm = R.front ? outward : mul(outward, -1.0);
      R.u = 0.0, R.v = 0.0;
      if (!(meta & kMoving)) {  // getSphereUv (hittable.zig:145-150)
        const D pi = 3.14159265358979323846;
        R.u = (rtwl::atan2(-outward.z, outward.x) + pi) / (2.0 * pi);
        R.v = rtwl::acos(-outward.y) / pi;
      }
      store_hit(A.out, i, hit_t, R, (uint32_t)hit_orig + 1u);
    }
  }
}

constexpr int kLanePacked = kFeatImage | kFeatLane | kFeatPacked, kLanePlain = kFeatImage | kFeatLane;
constexpr int kTriLanePacked = kLanePacked | kFeatTri, kTriLanePlain = kLanePlain | kFeatTri, kTriAll = kFeatAll | kFeatTri;

template <typename K>
int blocks_per_cu(K kernel, size_t lds) {
  int nb = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, kQueryBlock, lds);
  return (e == hipSuccess && nb > 0) ? nb : 1;
}

}  // namespace

size_t query_lds_bytes(int fs) {
  return (size_t)((fs & kFeatLane) ? (kLaneStackLds + kTravWords) * 64u : kBvhStack) * (kQueryBlock / 64) *
         sizeof(uint32_t);
}

hipError_t launch_world_query(const WorldQueryArgs& a, uint32_t grid, int fs, bool occlusion, hipStream_t s) {
  const size_t lds = query_lds_bytes(fs);
  const dim3 g(grid), b(kQueryBlock);
  if (fs == kLanePacked) {
    if (occlusion)
      hipLaunchKernelGGL((world_query_lane_kernel<kLanePacked, true>), g, b, lds, s, a);
    else
      hipLaunchKernelGGL((world_query_lane_kernel<kLanePacked, false>), g, b, lds, s, a);
  } else if (fs == kLanePlain) {
    if (occlusion)
      hipLaunchKernelGGL((world_query_lane_kernel<kLanePlain, true>), g, b, lds, s, a);
    else
      hipLaunchKernelGGL((world_query_lane_kernel<kLanePlain, false>), g, b, lds, s, a);
  } else if (fs == kTriLanePacked) {
    if (occlusion)
      hipLaunchKernelGGL((world_query_lane_kernel<kTriLanePacked, true>), g, b, lds, s, a);
    else
      hipLaunchKernelGGL((world_query_lane_kernel<kTriLanePacked, false>), g, b, lds, s, a);
  } else if (fs == kTriLanePlain) {
    if (occlusion)
      hipLaunchKernelGGL((world_query_lane_kernel<kTriLanePlain, true>), g, b, lds, s, a);
    else
      hipLaunchKernelGGL((world_query_lane_kernel<kTriLanePlain, false>), g, b, lds, s, a);
  } else if (fs == kTriAll) {
    if (occlusion)
      hipLaunchKernelGGL((world_query_kernel<kTriAll, true>), g, b, lds, s, a);
    else
      hipLaunchKernelGGL((world_query_kernel<kTriAll, false>), g, b, lds, s, a);
  } else {
    if (occlusion)
      hipLaunchKernelGGL((world_query_kernel<kFeatAll, true>), g, b, lds, s, a);
    else
      hipLaunchKernelGGL((world_query_kernel<kFeatAll, false>), g, b, lds, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_scene_query(const SceneQueryArgs& a, uint32_t grid, bool occlusion, hipStream_t s) {
  if (occlusion)
    hipLaunchKernelGGL(scene_query_kernel<true>, dim3(grid), dim3(kQueryBlock), 0, s, a);
  else
    hipLaunchKernelGGL(scene_query_kernel<false>, dim3(grid), dim3(kQueryBlock), 0, s, a);
  return hipGetLastError();
}

int query_blocks_per_cu(int fs, bool occlusion) {
  const size_t lds = query_lds_bytes(fs);
  if (fs == kLanePacked)
    return occlusion ? blocks_per_cu(world_query_lane_kernel<kLanePacked, true>, lds)
                     : blocks_per_cu(world_query_lane_kernel<kLanePacked, false>, lds);
  if (fs == kLanePlain)
    return occlusion ? blocks_per_cu(world_query_lane_kernel<kLanePlain, true>, lds)
                     : blocks_per_cu(world_query_lane_kernel<kLanePlain, false>, lds);
  if (fs == kTriLanePacked)
    return occlusion ? blocks_per_cu(world_query_lane_kernel<kTriLanePacked, true>, lds)
                     : blocks_per_cu(world_query_lane_kernel<kTriLanePacked, false>, lds);
  if (fs == kTriLanePlain)
    return occlusion ? blocks_per_cu(world_query_lane_kernel<kTriLanePlain, true>, lds)
                     : blocks_per_cu(world_query_lane_kernel<kTriLanePlain, false>, lds);
  if (fs == kTriAll)
    return occlusion ? blocks_per_cu(world_query_kernel<kTriAll, true>, lds)
                     : blocks_per_cu(world_query_kernel<kTriAll, false>, lds);
  return occlusion ? blocks_per_cu(world_query_kernel<kFeatAll, true>, lds)
                   : blocks_per_cu(world_query_kernel<kFeatAll, false>, lds);
}

}  // namespace rtwk
