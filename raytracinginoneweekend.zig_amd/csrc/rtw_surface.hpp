// rtw_surface.hpp — the host side of the surface queries (rtw_hip.h "surface
// queries"): the record's layout as the kernels store it and the
// argument check of the three entries.  No HIP: tests/native/surface_check.cpp
// builds it with a plain C++ compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "rtw_hip.h"

namespace rtws {

static_assert(sizeof(rtw_surface) == 64 && alignof(rtw_surface) == 8, "rtw_surface is 64 bytes, 8-byte aligned");
static_assert(offsetof(rtw_surface, fuzz) == 24 && offsetof(rtw_surface, ir) == 32 && offsetof(rtw_surface, kind) == 40 &&
                  offsetof(rtw_surface, mat) == 44 && offsetof(rtw_surface, tex) == 48 &&
                  offsetof(rtw_surface, tex_kind) == 52 && offsetof(rtw_surface, reserved) == 56,
              "the kernels store the record as eight 8-byte words");
static_assert(sizeof(rtw_hit) == 80 && sizeof(rtw_guide) == 32, "record sizes");

// Whether [a, a + na) and [b, b + nb) share a byte (either NULL or empty: no).
inline bool ranges_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && na && nb && x < y + nb && y < x + na;
}

// The checks the entries share, in the order the header lists them; `handle_ok`
// and n > 2^31 come first, then n == 0 (RTW_OK with *launch = false: nothing is
// read, so null buffers pass).  n <= 2^31 records of at most 80 bytes: no sum
// below wraps.
inline int check_call(const char* who, const void* d_hits, uint64_t n, const double* background, const void* d_surf,
                      const void* d_guides, bool* launch, std::string& msg) {
  *launch = false;
  auto fail = [&](const char* what) {
    msg = std::string(who) + ": " + what;
    return (int)RTW_EINVAL;
  };
  if (n > RTW_QUERY_MAX_RAYS) return fail("n > 2^31");
  if (n == 0) return RTW_OK;
  if (!d_hits) return fail("d_hits is NULL");
  if (!d_surf && !d_guides) return fail("d_surf and d_guides are both NULL");
  if (d_guides && !background) return fail("d_guides without a background");
  if (d_guides && !(std::isfinite(background[0]) && std::isfinite(background[1]) && std::isfinite(background[2])))
    return fail("the background is not finite");
  if ((((uintptr_t)d_hits | (uintptr_t)d_surf) & 7u) != 0) return fail("d_hits or d_surf is not 8-byte aligned");
  if (((uintptr_t)d_guides & 15u) != 0) return fail("d_guides is not 16-byte aligned");
  if (ranges_overlap(d_surf, n * sizeof(rtw_surface), d_hits, n * sizeof(rtw_hit)) ||
      ranges_overlap(d_guides, n * sizeof(rtw_guide), d_hits, n * sizeof(rtw_hit)))
    return fail("an output overlaps d_hits");
  if (ranges_overlap(d_surf, n * sizeof(rtw_surface), d_guides, n * sizeof(rtw_guide)))
    return fail("d_surf and d_guides overlap");
  *launch = true;
  return RTW_OK;
}

}  // namespace rtws
