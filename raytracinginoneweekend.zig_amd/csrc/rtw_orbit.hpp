// rtw_orbit.hpp — frames of a moving world for the CLI (rtw_render --frames N
// --orbit DEG): the world is uploaded once with RTW_WORLD_DYNAMIC and updated
// in place per frame (rtw_hip.h "dynamic worlds"; rtw_world_capi.hip).
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

#include "rtw_hip.h"

namespace rtw {

// Frame k of `frames` (k = 0 is the description as it stands): every sphere
// centre (both ends of a moving sphere) turned by k * deg degrees about the y
// axis, every RotateY op's angle advanced by as much — spheres orbit the
// scene's axis, boxes turn in place.  on_frame gets each frame's RGB8 image.
// rebuild_above >= 0: after a frame's update, when rtw_world_bvh_cost exceeds
// rebuild_above times its value right after the creation or the last rebuild,
// the frame's numbers go through rtw_world_rebuild, and one stderr line gives
// the frame and the cost before and after.
// on_guides (optional; rtw_render --aov-dir): each frame's feature buffers, W * H records in row-major order,
// from the frame's feature rays, their first hits and rtw_world_surface_device (frameGuides' pipeline on the
// updated world).  Without it nothing of that runs.
using FrameFn = std::function<void(uint32_t frame, const std::vector<uint8_t>& rgb)>;
using GuideFn = std::function<void(uint32_t frame, const std::vector<rtw_guide>& guides)>;
void renderOrbit(const rtw_camera& cam, const rtw_params& p, const rtw_world_desc& desc, uint32_t frames, double deg,
                 const FrameFn& on_frame, double rebuild_above = -1.0, const GuideFn& on_guides = GuideFn());

// The feature buffers of one frame of a world description: rtw_pixel_rays_device, rtw_world_trace_device and
// rtw_world_surface_device (guides only) on the current device — rtw_world_guides_device's bytes.
std::vector<rtw_guide> frameGuides(const rtw_camera& cam, uint32_t width, uint32_t height, const double background[3],
                                   const rtw_world_desc& desc);

// The same frames, accumulated over time (rtw_hip.h "temporal accumulation"; rtw_render --frames N
// --temporal): frame k renders with seed p.seed + k; before its update the previous frame's numbers are
// kept on the device; after the render come the pixel rays, their first hits, the guides read off those
// hits (rtw_world_surface_device: rtw_world_guides_device's bytes without its second trace), the hits'
// previous points (time = the feature ray's) and rtw_temporal_device.  on_frame gets the accumulated
// mean quantised as a render's (frame 0, whose accumulated mean is the render's own: the render's image),
// or with `denoise` rtw_denoise_device's image of the accumulated mean and the temporal variance.
// A turn of 0 degrees reprojects nothing (no previous points).  Whole frames only (row_stride 1).
struct TemporalRun {
  uint32_t max_history = 0;  // rtw_temporal_opts.max_history (0 = default)
  bool denoise = false;
  rtw_denoise_opts dn{};
};
void renderOrbitTemporal(const rtw_camera& cam, const rtw_params& p, const rtw_world_desc& desc, uint32_t frames,
                         double deg, const FrameFn& on_frame, const TemporalRun& run, double rebuild_above = -1.0,
                         const GuideFn& on_guides = GuideFn(), const rtw_temporal_clamp* clamp = nullptr,
                         const rtw_mirror_opts* mirror = nullptr);
// clamp (rtw_render --temporal-clamp G): every frame goes through rtw_temporal_clamped_device with it, the
// history clamped to the frame's neighbourhood; nullptr: rtw_temporal_device as before.
// mirror (rtw_render --temporal-mirror): the previous points come from rtw_world_mirror_points_device with
// it, a mirror's from where it showed the same reflected thing; nullptr:
// rtw_world_prev_points_device as before.

}  // namespace rtw
