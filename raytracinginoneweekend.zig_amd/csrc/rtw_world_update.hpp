// rtw_world_update.hpp — launches of the update kernels (rtw_world_update.hip)
// for rtw_world_update_device (rtw_world_capi.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "rtw_world_refit.hpp"

namespace rtwk {

struct UpdateArgs {
  rtwr::View v;      // device pointers
  double* partials;  // n_wg x rtwr::kPartial doubles (in the world's refit allocation)
  double* result;    // rtwr::kPartial doubles: the folded partial
  uint32_t n_wg;     // workgroups of the validation: ceil(max(n_prims, n_xforms, 1) / 256)
};

// Phase 1: reads the input only; leaves the folded rtwr::Partial in a.result.
hipError_t launch_update_validate(const UpdateArgs& a, hipStream_t s);
// Phase 2: records and transform values, then the nodes bottom-up: one launch
// per height below h_star, then one single-workgroup launch for the rest.
// h_off: rtwp::RefitPack::h_off (host).
hipError_t launch_update_commit(const UpdateArgs& a, const uint32_t* h_off, uint32_t h_max, uint32_t h_star, hipStream_t s);

}  // namespace rtwk
