// rtw_query_plan.hpp — what a ray query (rtw_hip.h "ray queries") derives on
// the host before its launch: the argument checks, the traversal after AUTO
// and the world's limits, and the launch geometry.  Host only, no HIP and no
// environment, like rtw_plan.hpp: tests/native/query_plan_check.cpp builds it
// with a plain C++ compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rtw_hip.h"

namespace rtwq {

constexpr uint32_t kBlock = 256;     // threads of a query workgroup (rtwk::kQueryBlock)
constexpr uint32_t kWaveRays = 64;   // rays of one wave step

// RTW_OK, or RTW_EINVAL with the message: null pointers, rays / hits not 8-byte
// aligned (out_align = 8; 1 for the occlusion bytes), n > RTW_QUERY_MAX_RAYS,
// a traversal that is not AUTO, UNION or LANE, flags != 0.
int check_batch(const char* who, const void* handle, const void* rays, uint64_t n, const rtw_query_opts* opts,
                const void* out, uint32_t out_align, std::string& msg);

// The walk a query of a world runs: LINEAR without a BVH; LANE where the world
// can walk per lane (lane_ok) and the caller forces it, or AUTO finds at least
// RTW_QUERY_LANE_NODES nodes; else UNION.
uint32_t traversal(uint32_t asked, uint32_t n_nodes, bool lane_ok);

// Workgroups of the launch: one 64-ray step per wave up to the device's resident workgroups (the
// kernels stride over the rest), at least 1.
uint32_t grid(uint64_t n, uint32_t cus, uint32_t blocks_per_cu);

}  // namespace rtwq
