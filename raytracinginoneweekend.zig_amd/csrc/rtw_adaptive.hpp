// rtw_adaptive.hpp — the per-pixel convergence criterion of adaptive sampling
// (rtw_hip.h rtw_accum_set_adaptive).  No HIP here: the
// accumulator's kernels (rtw_accum.hip) and the native check
// (tests/native/adaptive_check.cpp) compile the same function.
//
// A pixel holds cnt samples, m = cnt / chunk full chunks of them, and the
// statistic {SY, SY2} = {sum Y, sum Y^2} of the full chunks' luminances (Y =
// luminance of a chunk SUM).  se2 is the squared standard error of the pixel's
// mean luminance — rtw_accum_noise's per-pixel term — and the pixel has
// converged when it is at most thr = tol * tol (an absolute target).
// One IEEE operation per operator, in this order (-ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTW_ADAPT_HD __host__ __device__
#else
#define RTW_ADAPT_HD
#endif

namespace rtwa {

// se2 of a pixel with m >= 2 full chunks of `chunk` samples.
RTW_ADAPT_HD inline double pixel_se2(double sy, double sy2, uint32_t m, uint32_t chunk) {
  const double var = fmax(0.0, sy2 - sy * sy / (double)m);
  return var / ((double)m * (double)(m - 1) * (double)chunk * (double)chunk);
}

RTW_ADAPT_HD inline bool pixel_converged(double sy, double sy2, uint32_t cnt, uint32_t chunk, uint32_t min_spp,
                                         double thr) {
  const uint32_t m = cnt / chunk;
  if (m < 2 || cnt < min_spp) return false;
  return pixel_se2(sy, sy2, m, chunk) <= thr;
}

}  // namespace rtwa
