// rtw_world_update.hip — kernels of rtw_world_update_device (rtw_hip.h
// "dynamic worlds"): an uploaded world's primitives take new
// numbers in place and its BVH is refitted bottom-up.  The per-item steps are
// rtw_world_refit.hpp's, the ones the host refit (rtw_world_refit.cpp) runs,
// so the device tables equal the host's byte for byte.
//
// Visibility between tree heights comes from kernel boundaries, and inside the
// last launch from the workgroup barrier: no workgroup reads what another
// wrote in the same launch, there are no counters and nothing spins.
#include "rtw_tri.hpp"
#include "rtw_world_update.hpp"

namespace rtwk {
namespace {

using rtwr::kBlock;

// Folds the workgroup's partials in LDS; lane 0 holds the result.
__device__ void block_fold(rtwr::Partial& p, double (*sh)[rtwr::kPartial]) {
  const uint32_t t = threadIdx.x;
  rtwr::partial_store(p, sh[t]);
  __syncthreads();
  for (uint32_t step = kBlock / 2; step > 0; step /= 2) {
    if (t < step) {
      rtwr::Partial q;
      rtwr::partial_load(q, sh[t + step]);
      rtwr::partial_fold(p, q);
      rtwr::partial_store(p, sh[t]);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void wu_validate(UpdateArgs a) {
  __shared__ double sh[kBlock][rtwr::kPartial];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  rtwr::Partial p;
  rtwr::partial_init(p);
  if (i < a.v.n_prims) rtwr::validate_prim(a.v, i, p);
  if (i < a.v.n_xforms) rtwr::validate_xform(a.v, i, p);
  block_fold(p, sh);
  if (threadIdx.x == 0) rtwr::partial_store(p, a.partials + (size_t)rtwr::kPartial * blockIdx.x);
}

__global__ __launch_bounds__(256) void wu_reduce(UpdateArgs a) {
  __shared__ double sh[kBlock][rtwr::kPartial];
  rtwr::Partial p;
  rtwr::partial_init(p);
  for (uint32_t w = threadIdx.x; w < a.n_wg; w += kBlock) {
    rtwr::Partial q;
    rtwr::partial_load(q, a.partials + (size_t)rtwr::kPartial * w);
    rtwr::partial_fold(p, q);
  }
  block_fold(p, sh);
  if (threadIdx.x == 0) rtwr::partial_store(p, a.result);
}

__global__ __launch_bounds__(256) void wu_records(UpdateArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < a.v.n_prims) rtwr::commit_prim(a.v, i);
  if (i < a.v.n_xforms) rtwr::commit_xform(a.v, i);
}

// Entries [begin, begin + count) of by_height, whose heights lie in
// [h_lo, h_hi].  h_lo < h_hi only in a single-workgroup launch: a height reads
// the plain bounds the height below wrote, after the barrier.
__global__ __launch_bounds__(256) void wu_nodes(UpdateArgs a, uint32_t begin, uint32_t count, uint32_t h_lo, uint32_t h_hi) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool mine = i < count;
  const uint32_t n = mine ? a.v.by_height[begin + i] : 0u, my_h = mine ? a.v.heights[begin + i] : 0u;
  for (uint32_t h = h_lo; h <= h_hi; ++h) {
    if (mine && my_h == h) rtwr::commit_node(a.v, n);
    if (h < h_hi) __syncthreads();
  }
}

}  // namespace

hipError_t launch_update_validate(const UpdateArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(wu_validate, dim3(a.n_wg), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(wu_reduce, dim3(1), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_update_commit(const UpdateArgs& a, const uint32_t* h_off, uint32_t h_max, uint32_t h_star, hipStream_t s) {
  hipLaunchKernelGGL(wu_records, dim3(a.n_wg), dim3(kBlock), 0, s, a);
  if (a.v.n_nodes) {
    for (uint32_t h = 1; h < h_star; ++h) {
      const uint32_t begin = h_off[h - 1], count = h_off[h] - begin;
      if (count) hipLaunchKernelGGL(wu_nodes, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, s, a, begin, count, h, h);
    }
    const uint32_t begin = h_off[h_star - 1], count = a.v.n_nodes - begin;  // <= 256 nodes: one workgroup
    hipLaunchKernelGGL(wu_nodes, dim3(1), dim3(kBlock), 0, s, a, begin, count, h_star, h_max);
  }
  return hipGetLastError();
}

}  // namespace rtwk
