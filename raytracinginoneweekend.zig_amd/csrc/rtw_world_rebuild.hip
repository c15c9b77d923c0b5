// rtw_world_rebuild.hip — kernels of rtw_world_rebuild_device and
// rtw_world_bvh_cost (rtw_hip.h "dynamic worlds"): an uploaded
// world gets a new tree from new numbers.  Keys, splits, numbering and the
// schedule are rtw_world_build.hpp's, the ones the host build
// (rtw_world_build.cpp) runs, so the device tables equal the host's byte for
// byte; bounds and pretest records come from the refit's commit kernels
// (rtw_world_update.hip) run over the new tree.
//
// Visibility between stages comes from kernel boundaries, and between the
// levels of the topology kernel (one workgroup) from the workgroup barrier: no
// workgroup reads what another wrote in the same launch, there are no counters
// and nothing spins.  The sort is rocPRIM's radix sort (stable: ties keep list
// order), its temporary storage inside the world's rebuild allocation.
#include "rtw_world_rebuild.hpp"

#include <rocprim/device/device_radix_sort.hpp>

namespace rtwk {
namespace {

using rtwr::kBlock;

__global__ __launch_bounds__(256) void rb_init(RebuildArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < a.v.n_prims) a.self[i] = i;
}

// Folds six doubles per lane (box minima, then maxima) in LDS; lane 0 holds the result.
__device__ void box_fold(double lo[3], double hi[3], double (*sh)[6]) {
  const uint32_t t = threadIdx.x;
  for (int c = 0; c < 3; ++c) sh[t][c] = lo[c], sh[t][3 + c] = hi[c];
  __syncthreads();
  for (uint32_t step = kBlock / 2; step > 0; step /= 2) {
    if (t < step) {
      lo[0] = rtwr::tmin(lo[0], sh[t + step][0]), lo[1] = rtwr::tmin(lo[1], sh[t + step][1]);
      lo[2] = rtwr::tmin(lo[2], sh[t + step][2]);
      hi[0] = rtwr::tmax(hi[0], sh[t + step][3]), hi[1] = rtwr::tmax(hi[1], sh[t + step][4]);
      hi[2] = rtwr::tmax(hi[2], sh[t + step][5]);
      sh[t][0] = lo[0], sh[t][1] = lo[1], sh[t][2] = lo[2], sh[t][3] = hi[0], sh[t][4] = hi[1], sh[t][5] = hi[2];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void rb_centroids(RebuildArgs a) {
  __shared__ double sh[kBlock][6];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  double lo[3] = {rtwr::inf(), rtwr::inf(), rtwr::inf()}, hi[3] = {-rtwr::inf(), -rtwr::inf(), -rtwr::inf()};
  if (i < a.v.n_prims) {
    double bl[3], bh[3], c[3];
    rtwr::box_of(a.v, rtwr::prim_meta0(a.v, a.v.order[i]), i, bl, bh);
    rtwb::centroid(bl, bh, c);
    lo[0] = hi[0] = c[0], lo[1] = hi[1] = c[1], lo[2] = hi[2] = c[2];
  }
  box_fold(lo, hi, sh);
  if (threadIdx.x == 0) {
    double* d = a.cpart + (size_t)6 * blockIdx.x;
    d[0] = lo[0], d[1] = lo[1], d[2] = lo[2], d[3] = hi[0], d[4] = hi[1], d[5] = hi[2];
  }
}

__global__ __launch_bounds__(256) void rb_centroid_fold(RebuildArgs a) {
  __shared__ double sh[kBlock][6];
  double lo[3] = {rtwr::inf(), rtwr::inf(), rtwr::inf()}, hi[3] = {-rtwr::inf(), -rtwr::inf(), -rtwr::inf()};
  for (uint32_t w = threadIdx.x; w < a.n_wg; w += kBlock) {
    const double* d = a.cpart + (size_t)6 * w;
    lo[0] = rtwr::tmin(lo[0], d[0]), lo[1] = rtwr::tmin(lo[1], d[1]), lo[2] = rtwr::tmin(lo[2], d[2]);
    hi[0] = rtwr::tmax(hi[0], d[3]), hi[1] = rtwr::tmax(hi[1], d[4]), hi[2] = rtwr::tmax(hi[2], d[5]);
  }
  box_fold(lo, hi, sh);
  if (threadIdx.x == 0)
    a.cbox[0] = lo[0], a.cbox[1] = lo[1], a.cbox[2] = lo[2], a.cbox[3] = hi[0], a.cbox[4] = hi[1], a.cbox[5] = hi[2];
}

__global__ __launch_bounds__(256) void rb_keys(RebuildArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.v.n_prims) return;
  const double clo[3] = {a.cbox[0], a.cbox[1], a.cbox[2]}, chi[3] = {a.cbox[3], a.cbox[4], a.cbox[5]};
  a.key[i] = rtwb::key_of(a.v, i, clo, chi);
}

// Exclusive scan of one value per lane over the workgroup; *total: the sum.
__device__ uint32_t block_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
  const uint32_t t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (uint32_t step = 1; step < rtwb::kTopoBlock; step *= 2) {
    const uint32_t add = t >= step ? sh[t - step] : 0u;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const uint32_t incl = sh[t];
  *total = sh[rtwb::kTopoBlock - 1];
  __syncthreads();
  return incl - v;
}

// One workgroup: the splits level by level over a compacted worklist (the
// nodes of a level are consecutive records; a node's range is rng[2 x]), the
// next level's records from an exclusive scan of the interior-child counts,
// then the schedule.  Every index stays inside its table whatever the keys
// hold: a split lies strictly inside its range, so a tree over n primitives
// has n - 1 interior nodes.
__global__ __launch_bounds__(1024) void rb_topology(RebuildArgs a) {
  __shared__ uint32_t sh[rtwb::kTopoBlock];
  __shared__ uint32_t level_off[rtwb::kMaxLevels + 1];
  const uint32_t t = threadIdx.x, n = a.v.n_prims, nn = a.v.n_nodes, cap = rtwb::cap_of(n);
  if (t == 0) a.rng[0] = 0u, a.rng[1] = n, level_off[0] = 0u;
  __syncthreads();
  uint32_t begin = 0, count = 1, depth = 0;
  while (count != 0u && depth < rtwb::kMaxLevels) {
    const uint32_t next = begin + count;
    uint32_t made = 0;
    for (uint32_t chunk = 0; chunk < count; chunk += rtwb::kTopoBlock) {
      const uint32_t x = begin + chunk + t;
      const bool mine = chunk + t < count;
      uint32_t b = 0, m = 0, e = 0, kids = 0;
      if (mine) {
        b = a.rng[2 * (size_t)x], e = a.rng[2 * (size_t)x + 1];
        m = rtwb::split_of(a.keys, b, e, depth, cap);
        kids = (m - b > 1u ? 1u : 0u) + (e - m > 1u ? 1u : 0u);
      }
      uint32_t total;
      uint32_t slot = next + made + block_scan(kids, sh, &total);
      if (mine) {
        uint32_t r0 = rtwb::leaf_ref(b), r1 = rtwb::leaf_ref(m);
        if (m - b > 1u && slot < nn) a.rng[2 * (size_t)slot] = b, a.rng[2 * (size_t)slot + 1] = m, r0 = slot++;
        if (e - m > 1u && slot < nn) a.rng[2 * (size_t)slot] = m, a.rng[2 * (size_t)slot + 1] = e, r1 = slot;
        a.refs[2 * (size_t)x] = r0, a.refs[2 * (size_t)x + 1] = r1;
      }
      made += total;
    }
    if (t == 0) a.levels[1 + depth] = count, level_off[depth + 1] = next;
    begin = next, count = made < nn - next ? made : nn - next, ++depth;  // (made <= nn - next: n - 1 nodes in all)
    __syncthreads();  // the next level reads the ranges this one wrote
  }
  if (t == 0) a.levels[0] = depth;
  for (uint32_t l = 0; l < depth; ++l)
    for (uint32_t x = level_off[l] + t; x < level_off[l + 1]; x += rtwb::kTopoBlock) {
      const uint32_t at = rtwb::sched_place(nn, level_off[l], level_off[l + 1], x);
      a.by_height[at] = x, a.heights[at] = rtwb::sched_label(depth, l);
    }
}

// Meta doubles of the primitive that moves to position `pos`, read at its old one.
__global__ __launch_bounds__(256) void rb_stage(RebuildArgs a) {
  const uint32_t pos = blockIdx.x * kBlock + threadIdx.x;
  if (pos >= a.v.n_prims) return;
  const double* s = a.v.prim + (size_t)kWorldRec * a.v.order[a.sorted[pos]];
  double* d = a.meta + (size_t)3 * pos;
  d[0] = s[11], d[1] = s[14], d[2] = s[15];
}

__device__ bool leaf_eligible(const RebuildArgs& a, uint32_t pos) {
  return rtwr::eligible(rtwr::ld_u32(a.meta + (size_t)3 * pos + 1, 0), a.v.a + (size_t)9 * a.sorted[pos]);
}

__global__ __launch_bounds__(256) void rb_apply(RebuildArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < a.v.n_prims) {  // position i
    double* d = a.v.prim + (size_t)kWorldRec * i;
    const double* m = a.meta + (size_t)3 * i;
    d[11] = m[0], d[14] = m[1], d[15] = m[2];
    const uint32_t li = a.sorted[i];
    const_cast<uint32_t*>(a.v.order)[li] = i;
    const bool el = leaf_eligible(a, i);
    const_cast<uint32_t*>(a.v.mate)[li] = el ? li : rtwr::kNone;
    if (a.v.has_table && !el)
      for (int k = 0; k < 16; ++k) a.v.cull[(size_t)16 * i + k] = 0.0f;
  }
  if (i < a.v.n_nodes) {  // node i, and entry i of the schedule
    uint32_t cd = 0;
    for (int c = 0; c < 2; ++c) {
      const uint32_t ref = a.refs[2 * (size_t)i + c];
      rtwr::st_u32(a.v.node + (size_t)kNodeWords * i, 12 + c, ref);
      if ((ref & kLeafBit) && leaf_eligible(a, ref & 0x7FFFFFu)) cd |= 1u << c;
    }
    const_cast<uint32_t*>(a.v.cand)[i] = cd;
    const_cast<uint32_t*>(a.v.by_height)[i] = a.by_height[i];
    const_cast<uint32_t*>(a.v.heights)[i] = a.heights[i];
  }
}

// Sums one double per lane in a fixed order; lane 0 holds the result.
__device__ double sum_fold(double v, double* sh) {
  const uint32_t t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (uint32_t step = kBlock / 2; step > 0; step /= 2) {
    if (t < step) v = v + sh[t + step], sh[t] = v;
    __syncthreads();
  }
  return v;
}

__global__ __launch_bounds__(256) void rb_cost(const float* node, uint32_t n_nodes, double* partials) {
  __shared__ double sh[kBlock];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const double v = sum_fold(i < n_nodes ? rtwb::node_cost(node + (size_t)kNodeWords * i) : 0.0, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = v;
}

__global__ __launch_bounds__(256) void rb_cost_fold(const float* node, uint32_t n_wg, const double* partials, double* out) {
  __shared__ double sh[kBlock];
  double v = 0.0;
  for (uint32_t w = threadIdx.x; w < n_wg; w += kBlock) v = v + partials[w];
  v = sum_fold(v, sh);
  if (threadIdx.x == 0) out[0] = v / rtwb::root_half_area(node);
}

}  // namespace

hipError_t rebuild_sort_bytes(uint32_t n_prims, size_t* bytes) {
  *bytes = 0;
  return rocprim::radix_sort_pairs(nullptr, *bytes, static_cast<uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                   static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), (size_t)n_prims, 0u,
                                   3u * rtwb::kFieldBits, hipStream_t(nullptr));
}

hipError_t launch_rebuild_init(const RebuildArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(rb_init, dim3((a.v.n_prims + kBlock - 1) / kBlock), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rebuild_build(const RebuildArgs& a, hipStream_t s) {
  const uint32_t wg = (a.v.n_prims + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(rb_centroids, dim3(wg), dim3(kBlock), 0, s, a);
  RebuildArgs f = a;
  f.n_wg = wg;
  hipLaunchKernelGGL(rb_centroid_fold, dim3(1), dim3(kBlock), 0, s, f);
  hipLaunchKernelGGL(rb_keys, dim3(wg), dim3(kBlock), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t bytes = a.sort_bytes;
  e = rocprim::radix_sort_pairs(a.sort_tmp, bytes, a.key, a.keys, a.self, a.sorted, (size_t)a.v.n_prims, 0u,
                                3u * rtwb::kFieldBits, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rb_topology, dim3(1), dim3(rtwb::kTopoBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rebuild_apply(const RebuildArgs& a, hipStream_t s) {
  const uint32_t wg = (a.v.n_prims + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(rb_stage, dim3(wg), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(rb_apply, dim3(wg), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_bvh_cost(const float* node, uint32_t n_nodes, double* partials, double* out, hipStream_t s) {
  const uint32_t wg = (n_nodes + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(rb_cost, dim3(wg), dim3(kBlock), 0, s, node, n_nodes, partials);
  hipLaunchKernelGGL(rb_cost_fold, dim3(1), dim3(kBlock), 0, s, node, wg, static_cast<const double*>(partials), out);
  return hipGetLastError();
}

}  // namespace rtwk
