// rtw_specular.hip — device side of the mirror points (rtw_hip.h "mirror
// points"): for each hit record its previous point, and for a
// record that counts as a mirror the point of the mirror that showed the same
// reflected thing in the previous frame.  The arithmetic is rtw_specular.hpp's
// and rtw_temporal.hpp's, the functions rtw_world_mirror_points_host runs; the
// reflected ray is walked by the ray queries' own walks (rtw_world_walk.hpp)
// and its record is rtw_world_trace_device's, so the device's bytes are the
// host pipeline's.
//
// Two kernels, the query kernels' shapes (rtw_query.hip): the linear loop /
// union walk with one record per lane and a grid-stride over the batch, where a
// wave walks for its mirror lanes only; and the per-lane walk with lane-level
// regeneration, where a record that needs no walk (a miss, a surface that is no
// mirror) is finished at once and its lane takes the wave's next record, until
// every lane of the wave walks a reflected ray or the records ran out.  LDS: the
// walks' own stacks.  No scratch, no atomics, no workspace.
// -ffp-contract=off (Makefile).
#include <hip/hip_runtime.h>

#include "rtw_device.hpp"
#include "rtw_libm.hpp"
#include "rtw_query_dev.hpp"
#include "rtw_specular.hpp"
#include "rtw_world_walk.hpp"

namespace rtwk {

namespace {

constexpr D kInf = (D)__builtin_huge_val();

// What prev_point and prev_normal read of a primitive (prev_points_kernel's rule).
// rec: its stored record; prim: its list index + 1.
struct PrimPrev {
  double r[11];
  uint32_t kind, xf_h;
  const double *v_now, *v_prev;
};
__device__ __forceinline__ PrimPrev prim_prev(const WorldMirrorArgs& A, const double* rec, uint32_t prim) {
  PrimPrev q;
  const uint32_t meta0 = rtwr::ld_u32(rec + 14, 0);
  const uint32_t xf = meta0 >> 8;  // transform index + 1
  q.kind = meta0 & 0xFFu;
  if (A.a_prev) {  // (uniform)
    rtwr::fill_record(q.kind, A.a_prev + (size_t)9 * (prim - 1u), q.r);
  } else {
#pragma unroll
    for (int k = 0; k < 11; ++k) q.r[k] = k < 9 ? rec[k] : 0.0;
  }
  q.xf_h = 0u;
  q.v_now = rec, q.v_prev = rec;  // (not read without a chain)
  if (xf) {
    const double* x = A.q.w.xform + (size_t)kWorldRec * (xf - 1u);
    q.xf_h = rtwr::ld_u32(x, 0);
    q.v_now = x + 4;
    q.v_prev = A.xv_prev ? A.xv_prev + (size_t)3 * kMaxXfOps * (xf - 1u) : q.v_now;
  }
  return q;
}

__device__ __forceinline__ void store_point(double* out, uint64_t i, double x, double y, double z) {
  double* o = out + 3 * i;
  o[0] = x, o[1] = y, o[2] = z;
}

// Record i (< n).  A miss or a surface that is no mirror: its previous point
// (rtw_world_prev_points_device's bytes) and a zero reflected record are
// written, false.  A mirror: q = its reflected ray, true.
__device__ __forceinline__ bool mirror_begin(const WorldMirrorArgs& A, uint64_t i, QRay& q) {
  const WorldView& W = A.q.w;
  const double* h = A.hits + 10 * i;
  const uint64_t pf = reinterpret_cast<const uint64_t*>(h)[9];
  const uint32_t prim = (uint32_t)pf, front = (uint32_t)(pf >> 32);
  if (prim == 0u || prim > W.n_prims) {
    store_point(A.prev_p, i, 0.0, 0.0, 0.0);
    if (A.q.out) store_miss(A.q.out, i);  // (uniform)
    return false;
  }
  const double* rec = W.prim + (size_t)kWorldRec * W.order[prim - 1u];
  const uint32_t* mt = meta_of(rec);
  const uint32_t mat_kind = *reinterpret_cast<const uint32_t*>(W.mat + (size_t)8 * mt[1]);
  const double p[3] = {h[1], h[2], h[3]}, nrm[3] = {h[4], h[5], h[6]};
  if (!rtwsp::is_mirror(prim, W.n_prims, front, mt[0] & 0xFFu, mat_kind)) {
    const PrimPrev pp = prim_prev(A, rec, prim);
    double m[3];
    rtwt::prev_point(p, nrm, h[7], h[8], front, pp.kind, pp.r, pp.xf_h, pp.v_now, pp.v_prev, A.q.rays[9 * i + 6],
                     A.a_prev || A.xv_prev, m);
    store_point(A.prev_p, i, m[0], m[1], m[2]);
    if (A.q.out) store_miss(A.q.out, i);
    return false;
  }
  const double* r = A.q.rays + 9 * i;
  const double ray[9] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]};
  double r2[9];
  rtwsp::reflect_ray(ray, p, nrm, r2);
  q.o = mk(r2[0], r2[1], r2[2]);
  q.d = mk(r2[3], r2[4], r2[5]);
  q.time = r2[6];  // (t_min, t_max: rtwsp::kReflTmin and +inf, the kernels' constants)
  return true;
}

// A mirror lane's finished walk of its reflected ray q: the NaN fallback
// (finish_ray's), the reflected record, the target and the mirror point.
template <int FEAT>
__device__ __forceinline__ void mirror_finish(const WorldMirrorArgs& A, uint64_t i, const QRay& q, WHit& h) {
  const WorldView& W = A.q.w;
  if (__builtin_expect(h.nan != 0u, 0)) seq_hit<FEAT>(W, W.order, q.o, q.d, q.time, rtwsp::kReflTmin, h, kInf);
  const bool moved = A.a_prev || A.xv_prev;  // (uniform)
  const bool tsky = h.pos < 0;
  double tg[3];
  if (tsky) {
    if (A.q.out) store_miss(A.q.out, i);
    const rtwsp::V3 u = rtwsp::unit(rtwsp::v3(q.d.x, q.d.y, q.d.z));
    tg[0] = u.x, tg[1] = u.y, tg[2] = u.z;
  } else {
    const HitRec R = hit_record<FEAT>(W, h.pos, h.t, q.o, q.d, q.time, true);
    const uint32_t prim2 = (uint32_t)h.orig + 1u;
    if (A.q.out) store_hit(A.q.out, i, h.t, R, prim2);
    const PrimPrev p2 = prim_prev(A, W.prim + (size_t)kWorldRec * (uint32_t)h.pos, prim2);
    const double p[3] = {R.p.x, R.p.y, R.p.z}, nrm[3] = {R.nrm.x, R.nrm.y, R.nrm.z};
    rtwt::prev_point(p, nrm, R.u, R.v, R.front ? 1u : 0u, p2.kind, p2.r, p2.xf_h, p2.v_now, p2.v_prev, q.time, moved, tg);
  }
  // the mirror's own record again (a mirror: prim is of the list, front == 1)
  const double* hr = A.hits + 10 * i;
  const uint32_t prim = (uint32_t)reinterpret_cast<const uint64_t*>(hr)[9];
  const PrimPrev pp = prim_prev(A, W.prim + (size_t)kWorldRec * W.order[prim - 1u], prim);
  const double p[3] = {hr[1], hr[2], hr[3]}, nrm[3] = {hr[4], hr[5], hr[6]};
  double Mg[3], ng[3], m[3];
  rtwt::prev_point(p, nrm, hr[7], hr[8], 1u, pp.kind, pp.r, pp.xf_h, pp.v_now, pp.v_prev, q.time, moved, Mg);
  rtwsp::prev_normal(nrm, pp.xf_h, pp.v_now, pp.v_prev, moved, ng);
  store_point(A.prev_p, i, Mg[0], Mg[1], Mg[2]);  // (first, so that Mg need not stay in registers)
  if (rtwsp::mirror_point(pp.kind, Mg, ng, pp.r[6], A.cam_o, tsky, tg, A.steps, m)) store_point(A.prev_p, i, m[0], m[1], m[2]);
}

// Linear loop / union walk: 64 records per wave step, grid-stride over the batch.
template <int FEAT>
__global__ void __launch_bounds__(kQueryBlock) world_mirror_kernel(WorldMirrorArgs A) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  uint32_t* stack = reinterpret_cast<uint32_t*>(lds_raw) + (threadIdx.x >> 6) * kBvhStack;  // this wave's
  const WorldView& W = A.q.w;
  const uint32_t lid = lane_id();
  const uint64_t waves = (uint64_t)gridDim.x * (kQueryBlock / 64);
  unsigned long long nv = 0, nt = 0;
  KStats st;
  for (uint64_t base = ((uint64_t)blockIdx.x * (kQueryBlock / 64) + (threadIdx.x >> 6)) * 64u; base < A.q.n;
       base += waves * 64u) {  // (wave-uniform)
    const uint64_t i = base + lid;
    QRay q;
    if (i < A.q.n && mirror_begin(A, i, q)) {
      WHit h;
      closest<0, FEAT, false, true>(W, ray_margin(A.q.reach, q.o), stack, q.o, q.d, q.time, rtwsp::kReflTmin, h, nv, nt, st, kInf);
      if (A.q.seq_times && (q.time < 0.0 || q.time > 1.0)) h.nan = 1u, h.pos = -1;
      mirror_finish<FEAT>(A, i, q, h);
    }
  }
}

// Per-lane walk (sphere worlds with a BVH): world_query_lane_kernel's order of
// records (wave w takes the 64-record blocks w, w + waves, ...), with the
// hand-out repeated until every lane walks or none are left.
template <int FEAT>
__global__ void __launch_bounds__(kQueryBlock, 4) world_mirror_lane_kernel(WorldMirrorArgs A) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  constexpr uint32_t kWaveWords = (kLaneStackLds + kTravWords) * 64u;
  uint32_t* stack = reinterpret_cast<uint32_t*>(lds_raw) + (threadIdx.x >> 6) * kWaveWords;
  LaneTravRows* rows = reinterpret_cast<LaneTravRows*>(stack + kLaneStackLds * 64u);
  const WorldView& W = A.q.w;
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
  auto rec_index = [&](uint32_t k) -> uint64_t { return ((wave + (uint64_t)(k >> 6) * waves) << 6) + (k & 63u); };
  uint32_t k = 0;  // (wave-uniform) records of this wave handed out
  bool walking = false, done = false;
  uint32_t mine = 0;  // (n <= 2^31)
  QRay q;
  q.o = mk(0.0, 0.0, 0.0), q.d = mk(1.0, 1.0, 1.0), q.time = 0.0, q.tmin = 0.0, q.tmax = 0.0;
  unsigned long long nv = 0, nt = 0, wi = 0, wl = 0;
  for (;;) {
    for (;;) {  // (wave-uniform) a lane whose record needed no walk asks again
      const bool need = !walking && !done;
      const uint64_t nm = wballot(need);
      if (!nm) break;
      if (need) {
        const uint64_t i = rec_index(k + mbcnt64(nm));
        if (i >= A.q.n) {
          done = true;  // (indices grow with k: so are this lane's later ones)
        } else if (mirror_begin(A, i, q)) {
          mine = (uint32_t)i;
          trav_begin(rows, lid, kInf);
          walking = true;
        }
      }
      k += popc64(nm);
    }
    if (!wany(walking)) break;
    const uint32_t yl = rec_index(k) < A.q.n ? A.q.lane_yield : 0u;  // nothing to take: walk to the end
    WHit h;
    if (trav_phase<0, FEAT, false, true>(W, ray_margin(A.q.reach, q.o), stack, rows, node_cache, lid, walking, yl, q.o, q.d,
                                         q.time, rtwsp::kReflTmin, h, nv, nt, wi, wl)) {
      walking = false;
      if (A.q.seq_times && (q.time < 0.0 || q.time > 1.0)) h.nan = 1u, h.pos = -1;
      mirror_finish<FEAT>(A, mine, q, h);
    }
  }
}

constexpr int kLanePacked = kFeatImage | kFeatLane | kFeatPacked, kLanePlain = kFeatImage | kFeatLane;

template <typename K>
int blocks_per_cu(K kernel, size_t lds) {
  int nb = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, kQueryBlock, lds);
  return (e == hipSuccess && nb > 0) ? nb : 1;
}

}  // namespace

hipError_t launch_world_mirror(const WorldMirrorArgs& a, uint32_t grid, int fs, hipStream_t s) {
  const size_t lds = query_lds_bytes(fs);
  const dim3 g(grid), b(kQueryBlock);
  if (fs == kLanePacked)
    hipLaunchKernelGGL((world_mirror_lane_kernel<kLanePacked>), g, b, lds, s, a);
  else if (fs == kLanePlain)
    hipLaunchKernelGGL((world_mirror_lane_kernel<kLanePlain>), g, b, lds, s, a);
  else
    hipLaunchKernelGGL((world_mirror_kernel<kFeatAll>), g, b, lds, s, a);
  return hipGetLastError();
}

int mirror_blocks_per_cu(int fs) {
  const size_t lds = query_lds_bytes(fs);
  if (fs == kLanePacked) return blocks_per_cu(world_mirror_lane_kernel<kLanePacked>, lds);
  if (fs == kLanePlain) return blocks_per_cu(world_mirror_lane_kernel<kLanePlain>, lds);
  return blocks_per_cu(world_mirror_kernel<kFeatAll>, lds);
}

}  // namespace rtwk
