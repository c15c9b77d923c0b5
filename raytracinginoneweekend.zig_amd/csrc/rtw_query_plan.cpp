// rtw_query_plan.cpp — rtw_query_plan.hpp, and the host helper rtw_pixel_ray.
#include "rtw_query_plan.hpp"

#include <algorithm>
#include <limits>

namespace rtwq {

int check_batch(const char* who, const void* handle, const void* rays, uint64_t n, const rtw_query_opts* opts,
                const void* out, uint32_t out_align, std::string& msg) {
  const std::string w(who);
  if (!handle || !rays || !out) {
    msg = w + ": world/scene, rays or output is NULL";
    return RTW_EINVAL;
  }
  if ((reinterpret_cast<uintptr_t>(rays) & 7u) != 0) {
    msg = w + ": rays are not 8-byte aligned";
    return RTW_EINVAL;
  }
  if ((reinterpret_cast<uintptr_t>(out) & (uintptr_t)(out_align - 1u)) != 0) {
    msg = w + ": output is not " + std::to_string(out_align) + "-byte aligned";
    return RTW_EINVAL;
  }
  if (n > RTW_QUERY_MAX_RAYS) {
    msg = w + ": " + std::to_string(n) + " rays, at most 2^31 per call";
    return RTW_EINVAL;
  }
  if (opts && (opts->traversal > RTW_WORLD_TRAVERSAL_LANE || opts->flags != 0)) {
    msg = w + ": opts.traversal " + std::to_string(opts->traversal) + " / flags " + std::to_string(opts->flags);
    return RTW_EINVAL;
  }
  return RTW_OK;
}

uint32_t traversal(uint32_t asked, uint32_t n_nodes, bool lane_ok) {
  if (n_nodes == 0) return RTW_WORLD_TRAVERSAL_LINEAR;
  const bool lane = lane_ok && (asked == RTW_WORLD_TRAVERSAL_LANE ||
                                (asked == RTW_WORLD_TRAVERSAL_AUTO && n_nodes >= RTW_QUERY_LANE_NODES));
  return lane ? RTW_WORLD_TRAVERSAL_LANE : RTW_WORLD_TRAVERSAL_UNION;
}

uint32_t grid(uint64_t n, uint32_t cus, uint32_t blocks_per_cu) {
  const uint64_t want = (n + kBlock - 1) / kBlock;
  const uint64_t cap = std::max<uint64_t>(1, (uint64_t)cus * blocks_per_cu);
  return (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
}

}  // namespace rtwq

extern "C" int rtw_pixel_ray(const rtw_camera* cam, uint32_t width, uint32_t height, uint32_t x, uint32_t y,
                             rtw_ray* out) {
  if (!cam || !out || width < 2 || height < 2 || x >= width || y >= height) return RTW_EINVAL;
  // Camera.getRay (main.zig:91-100) with its draws at their means (rtw_guides.hpp guide_ray)
  const double s = ((double)x + 0.5) / (double)(width - 1u);
  const double t = ((double)(height - 1u - y) + 0.5) / (double)(height - 1u);
  for (int k = 0; k < 3; ++k) {
    out->origin[k] = cam->origin[k];
    out->dir[k] = ((cam->lower_left_corner[k] + cam->horizontal[k] * s) + cam->vertical[k] * t) - cam->origin[k];
  }
  out->time = cam->time0 + 0.5 * (cam->time1 - cam->time0);
  out->t_min = 0.001;
  out->t_max = std::numeric_limits<double>::infinity();
  return RTW_OK;
}
