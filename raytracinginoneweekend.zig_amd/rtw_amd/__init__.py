"""rtw_amd — Python binding of the MI355X path tracer's C ABI (include/rtw_hip.h).

The product path is lib/librtw_hip.so (HIP kernels for gfx950 + host helpers).
This module only marshals plain arrays through ctypes; there is NO CPU
fallback: if the library is missing or no GPU is visible, calls fail loudly.

Reference correspondence (nsfisis/RayTracingInOneWeekend.zig):
  camera_init   -> Camera.init          src/main.zig:52-89
  image_height  -> main.zig:306
  cover_scene   -> generateRandomScene  src/main.zig:157-221 (DefaultPrng.init(seed), main.zig:300)
  render        -> the render loop      src/main.zig:378-402 (+ rayColor :103-122)
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)                      # raytracinginoneweekend.zig_amd/
REPO = os.path.dirname(ROOT)
LIB_PATH = os.environ.get("RTW_LIB_PATH") or os.path.join(ROOT, "lib", "librtw_hip.so")  # (override: dev A/B)
HEADER_PATH = os.path.join(REPO, "include", "rtw_hip.h")

RTW_OK, RTW_EINVAL, RTW_UNSUPPORTED, RTW_EHIP, RTW_ENOMEM, RTW_ENODEV = 0, -1, -2, -3, -4, -5
LAMBERT_SOLID, LAMBERT_CHECKER, METAL, DIELECTRIC, DIFFUSE_LIGHT = 0, 1, 2, 3, 4
PRECISION = {"f64": 0, "f32": 1}
ENGINE = {"megakernel": 0, "wavefront": 1}
DEFAULT_WF_PATHS = 5 << 17  # rtw_hip.h RTW_DEFAULT_WF_PATHS
DEFAULT_WF_SETS = 2  # rtw_hip.h RTW_DEFAULT_WF_SETS (params.wf_sets overrides)
DEFAULT_WF_PASSES = 16  # rtw_hip.h RTW_DEFAULT_WF_PASSES (params.wf_passes overrides)
WF_DRAIN = {"samples": 0, "slots": 1, "none": 2}  # rtw_wf_drain
WF_FORM = {"fused": 0, "split": 1}  # rtw_wf_form
WORLD_FEATURES = {"auto": 0, "all": 1}  # rtw_world_features
WORLD_TRAVERSAL = {"auto": 0, "union": 1, "lane": 2}  # rtw_world_traversal
STATS_WORDS = 16  # rtw_hip.h RTW_STATS_WORDS
STAT_NAMES = ["samples", "segments", "f32_skips", "cand_wave_iters", "cand_lanes", "disc_ge0_lanes",
              "sphere_loop_wave_iters", "cull_survivor_lanes", "cull_exact_wave_iters", "drain_segments",
              "drain_samples", "cluster_wave_tests", "cluster_wave_skips", "drain_wave_iters", "primary_rounds",
              "primary_idle_lanes"]  # RTW_STAT_*
STAT_NAMES_EX = STAT_NAMES + ["primary_mask_popcount", "tail_helped_samples", "tail_wave_iters",
                              "tail_idle_lane_iters", "untraced_units", "untraced_samples", "queue_claims",
                              "beam_passes"]  # rtw_render_stats_ex: word 16 on (24 = RTW_STATS_WORDS_EX)
DEFAULT_CHUNK = 20
COVER_BACKGROUND = (0.70, 0.80, 1.00)


class RtwError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"rtw status {status}: {msg}")
        self.status = status


class Material(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("reserved", C.c_uint32), ("albedo", C.c_double * 3),
                ("albedo_odd", C.c_double * 3), ("fuzz", C.c_double), ("ir", C.c_double)]


class Sphere(C.Structure):
    _fields_ = [("c0", C.c_double * 3), ("c1", C.c_double * 3), ("radius", C.c_double),
                ("t0", C.c_double), ("t1", C.c_double), ("moving", C.c_uint32), ("mat", C.c_uint32)]


class Camera(C.Structure):
    _fields_ = [(n, C.c_double * 3) for n in
                ("origin", "horizontal", "vertical", "lower_left_corner", "u", "v", "w")] + \
               [("lens_radius", C.c_double), ("time0", C.c_double), ("time1", C.c_double)]


class Params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32),
                ("max_depth", C.c_uint32), ("seed", C.c_uint64), ("background", C.c_double * 3),
                ("row_begin", C.c_uint32), ("row_stride", C.c_uint32), ("row_count", C.c_uint32),
                ("chunk", C.c_uint32), ("precision", C.c_uint32), ("device", C.c_int32),
                ("engine", C.c_uint32), ("wf_paths", C.c_uint32),
                ("wf_sets", C.c_uint32), ("wf_drain", C.c_uint32), ("wf_form", C.c_uint32),
                ("world_waves", C.c_uint32), ("world_features", C.c_uint32), ("world_traversal", C.c_uint32),
                ("wf_bounces", C.c_uint32), ("wf_passes", C.c_uint32)]


class Guide(C.Structure):
    """rtw_guide: a pixel's first-hit features (32 bytes)."""
    _fields_ = [("normal", C.c_float * 3), ("depth", C.c_float), ("albedo", C.c_float * 3), ("prim", C.c_uint32)]


GUIDE_DTYPE = np.dtype([("normal", np.float32, 3), ("depth", np.float32), ("albedo", np.float32, 3),
                        ("prim", np.uint32)])
VAR_UNKNOWN, VAR_EMPTY = -1.0, -2.0  # rtw_hip.h RTW_VAR_*
DENOISE_NO_COLOR, DENOISE_DIRECT, DENOISE_SPATIAL_VAR = 1, 2, 4  # rtw_denoise_opts.flags


class Ray(C.Structure):
    """rtw_ray: a caller-supplied ray of a query (72 bytes)."""
    _fields_ = [("origin", C.c_double * 3), ("dir", C.c_double * 3), ("time", C.c_double), ("t_min", C.c_double),
                ("t_max", C.c_double)]


class Hit(C.Structure):
    """rtw_hit: the closest hit's record (80 bytes; a miss is all zero, prim = list index + 1)."""
    _fields_ = [("t", C.c_double), ("p", C.c_double * 3), ("normal", C.c_double * 3), ("u", C.c_double),
                ("v", C.c_double), ("prim", C.c_uint32), ("front", C.c_uint32)]


class QueryOpts(C.Structure):
    """rtw_query_opts: traversal (WORLD_TRAVERSAL, 0 = auto), flags (0)."""
    _fields_ = [("traversal", C.c_uint32), ("flags", C.c_uint32)]


class History(C.Structure):
    """rtw_history: a pixel's temporal accumulation record (32 bytes)."""
    _fields_ = [("mean", C.c_float * 3), ("len", C.c_float), ("m1", C.c_float), ("m2", C.c_float),
                ("depth", C.c_float), ("prim", C.c_uint32)]


class TemporalOpts(C.Structure):
    """rtw_temporal_opts: every field 0 = its default (32, 0.02, 4, 0)."""
    _fields_ = [("max_history", C.c_uint32), ("depth_tol", C.c_double), ("min_len_var", C.c_uint32),
                ("flags", C.c_uint32)]


class TemporalClamp(C.Structure):
    """rtw_temporal_clamp: every field 0 = its default (gamma 0.5, radius 1, reserved 0); 16 bytes."""
    _fields_ = [("gamma", C.c_double), ("radius", C.c_uint32), ("reserved", C.c_uint32)]


HISTORY_DTYPE = np.dtype([("mean", np.float32, 3), ("len", np.float32), ("m1", np.float32), ("m2", np.float32),
                          ("depth", np.float32), ("prim", np.uint32)])


def temporal_opts(max_history=0, depth_tol=0.0, min_len_var=0, flags=0) -> TemporalOpts:
    return TemporalOpts(max_history, depth_tol, min_len_var, flags)


def temporal_clamp(gamma=0.0, radius=0) -> TemporalClamp:
    return TemporalClamp(gamma, radius, 0)


class MirrorOpts(C.Structure):
    """rtw_mirror_opts: every field 0 = its default (2 Newton steps, no flags); 8 bytes."""
    _fields_ = [("steps", C.c_uint32), ("flags", C.c_uint32)]


MIRROR_PREDICT_ONLY = 1  # rtw_hip.h RTW_MIRROR_PREDICT_ONLY


def mirror_opts(steps=0, flags=0) -> MirrorOpts:
    return MirrorOpts(steps, flags)


RAY_DTYPE = np.dtype([("origin", np.float64, 3), ("dir", np.float64, 3), ("time", np.float64),
                      ("t_min", np.float64), ("t_max", np.float64)])
HIT_DTYPE = np.dtype([("t", np.float64), ("p", np.float64, 3), ("normal", np.float64, 3), ("u", np.float64),
                      ("v", np.float64), ("prim", np.uint32), ("front", np.uint32)])
QUERY_MAX_RAYS = 1 << 31  # rtw_hip.h RTW_QUERY_MAX_RAYS


class Surface(C.Structure):
    """rtw_surface: what the surface under a hit record is (64 bytes; a miss is all zero; kind, mat, tex and
    tex_kind are the enumeration value or index + 1)."""
    _fields_ = [("value", C.c_double * 3), ("fuzz", C.c_double), ("ir", C.c_double), ("kind", C.c_uint32),
                ("mat", C.c_uint32), ("tex", C.c_uint32), ("tex_kind", C.c_uint32), ("reserved", C.c_uint32 * 2)]


SURFACE_DTYPE = np.dtype([("value", np.float64, 3), ("fuzz", np.float64), ("ir", np.float64), ("kind", np.uint32),
                          ("mat", np.uint32), ("tex", np.uint32), ("tex_kind", np.uint32), ("reserved", np.uint32, 2)])


def query_opts(traversal="auto") -> QueryOpts:
    return QueryOpts(WORLD_TRAVERSAL[traversal] if isinstance(traversal, str) else int(traversal), 0)


class DenoiseOpts(C.Structure):
    """rtw_denoise_opts: every field 0 = its default."""
    _fields_ = [("levels", C.c_uint32), ("sigma_color", C.c_double), ("sigma_normal", C.c_double),
                ("sigma_depth", C.c_double), ("sigma_albedo", C.c_double), ("flags", C.c_uint32)]


def denoise_opts(levels=0, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0,
                 flags=0) -> DenoiseOpts:
    return DenoiseOpts(levels, sigma_color, sigma_normal, sigma_depth, sigma_albedo, flags)


_lib = None


def lib() -> C.CDLL:
    """Load lib/librtw_hip.so (built by `make -C raytracinginoneweekend.zig_amd`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() "
                           "(there is no CPU fallback for the render path)")
    # One HIP runtime per process: torch wheels bundle their own
    # libamdhip64.so.7 (same soname as /opt/rocm's).  Loading torch first makes
    # the dynamic loader bind this library to torch's copy, so torch's device
    # memory / streams and our kernels share one runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    L.rtw_abi_version.restype = C.c_int
    L.rtw_device_count.restype = C.c_int
    L.rtw_last_error.restype = C.c_char_p
    L.rtw_camera_init.argtypes = [P(Camera)] + [C.c_double * 3] * 3 + [C.c_double] * 6
    L.rtw_image_height.restype = C.c_uint32
    L.rtw_image_height.argtypes = [C.c_uint32, C.c_double]
    L.rtw_cover_scene.argtypes = [C.c_uint64, C.c_void_p, P(C.c_uint32), C.c_void_p, P(C.c_uint32),
                                  C.c_uint64 * 4]
    L.rtw_render.argtypes = [P(Camera), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, P(Params),
                             C.c_void_p, C.c_void_p]
    L.rtw_scene_create.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, P(C.c_void_p)]
    L.rtw_scene_destroy.argtypes = [C.c_void_p]
    L.rtw_workspace_bytes.restype = C.c_size_t
    L.rtw_workspace_bytes.argtypes = [P(Params)]
    L.rtw_timer_create.argtypes = [P(C.c_void_p)]
    L.rtw_timer_destroy.argtypes = [C.c_void_p]
    L.rtw_timer_elapsed_ms.argtypes = [C.c_void_p, P(C.c_float)]
    L.rtw_sclk_probe_begin.argtypes = [C.c_void_p, C.c_double, P(C.c_void_p)]
    L.rtw_sclk_probe_end.argtypes = [C.c_void_p, P(C.c_double)]
    L.rtw_render_device.argtypes = [C.c_void_p, P(Camera), P(Params), C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtw_render_counts.argtypes = [C.c_void_p, P(Camera), P(Params), C.c_void_p, C.c_size_t,
                                    C.c_uint64 * 4]
    L.rtw_render_counts_ex.argtypes = [C.c_void_p, P(Camera), P(Params), C.c_void_p, C.c_size_t,
                                       C.c_uint64 * 6]
    L.rtw_render_stats.argtypes = [C.c_void_p, P(Camera), P(Params), C.c_void_p, C.c_size_t,
                                   C.c_uint64 * STATS_WORDS]
    if hasattr(L, "rtw_render_stats_ex"):  # (an older A/B build has none)
        L.rtw_render_stats_ex.argtypes = [C.c_void_p, P(Camera), P(Params), C.c_void_p, C.c_size_t,
                                          P(C.c_uint64), C.c_uint32]
    if not hasattr(L, "rtw_accum_create"):  # (A/B timing may load an older build without the accumulator)
        _lib = L
        return L
    # progressive rendering (rtw_accum_*)
    L.rtw_accum_create.argtypes = [P(Params), P(C.c_void_p)]
    L.rtw_accum_destroy.argtypes = [C.c_void_p]
    L.rtw_accum_samples.argtypes = [C.c_void_p, P(C.c_uint32)]
    L.rtw_accum_workspace_bytes.restype = C.c_size_t
    L.rtw_accum_workspace_bytes.argtypes = [P(Params), C.c_uint32]
    L.rtw_accum_world_workspace_bytes.restype = C.c_size_t
    L.rtw_accum_world_workspace_bytes.argtypes = [C.c_void_p, P(Params), C.c_uint32]
    for f in (L.rtw_accum_render_device, L.rtw_accum_world_render_device):
        f.argtypes = [C.c_void_p, C.c_void_p, P(Camera), C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.rtw_accum_resolve_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtw_accum_noise.argtypes = [C.c_void_p, C.c_void_p, P(C.c_double)]
    L.rtw_accum_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtw_accum_load.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    if hasattr(L, "rtw_accum_set_mask"):  # adaptive sampling (an older A/B build has none)
        L.rtw_accum_set_mask.argtypes = [C.c_void_p, C.c_void_p]
        L.rtw_accum_set_adaptive.argtypes = [C.c_void_p, C.c_double, C.c_uint32]
        L.rtw_accum_active.argtypes = [C.c_void_p, P(C.c_uint32), P(C.c_uint32)]
        L.rtw_accum_read_counts.argtypes = [C.c_void_p, C.c_void_p]
        L.rtw_accum_load_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    if hasattr(L, "rtw_denoise_device"):  # feature-guided denoiser (an older A/B build has none)
        for f in (L.rtw_scene_guides_device, L.rtw_world_guides_device):
            f.argtypes = [C.c_void_p, P(Camera), P(Params), C.c_void_p, C.c_void_p]
        L.rtw_denoise_workspace_bytes.restype = C.c_size_t
        L.rtw_denoise_workspace_bytes.argtypes = [C.c_uint32, C.c_uint32, P(DenoiseOpts)]
        for f in (L.rtw_denoise_device, L.rtw_denoise_host):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, P(DenoiseOpts), C.c_void_p,
                          C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "rtw_denoise_spatial_variance_device"):  # (an older A/B build has none)
            for f in (L.rtw_denoise_spatial_variance_device, L.rtw_denoise_spatial_variance_host):
                f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, P(DenoiseOpts), C.c_void_p,
                              C.c_void_p]
        L.rtw_accum_variance_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rtw_accum_denoise_workspace_bytes.restype = C.c_size_t
        L.rtw_accum_denoise_workspace_bytes.argtypes = [C.c_void_p, P(DenoiseOpts)]
        L.rtw_accum_denoise_device.argtypes = [C.c_void_p, C.c_void_p, P(DenoiseOpts), C.c_void_p, C.c_size_t,
                                               C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "rtw_world_trace_device"):  # ray queries (an older A/B build has none)
        L.rtw_pixel_ray.argtypes = [P(Camera), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(Ray)]
        for f in (L.rtw_world_trace_device, L.rtw_world_occluded_device):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, P(QueryOpts), C.c_void_p, C.c_void_p]
        for f in (L.rtw_scene_trace_device, L.rtw_scene_occluded_device):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.rtw_world_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, P(QueryOpts), C.c_void_p]
        L.rtw_scene_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.rtw_world_query_info.argtypes = [C.c_void_p, P(QueryOpts), C.c_uint32 * 4]
    if hasattr(L, "rtw_world_update_device"):  # dynamic worlds (an older A/B build has none)
        L.rtw_world_update.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.rtw_world_update_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rtw_world_table_bytes.restype = C.c_size_t
        L.rtw_world_table_bytes.argtypes = [C.c_void_p]
        L.rtw_world_read_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float * 2, C.c_double * 6]
        L.rtw_world_refit_tables_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_size_t, C.c_float * 2, C.c_double * 6]
    if hasattr(L, "rtw_world_rebuild_device"):  # rebuilds and the tree cost
        L.rtw_world_rebuild.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.rtw_world_rebuild_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rtw_world_bvh_cost.argtypes = [C.c_void_p, C.c_void_p, P(C.c_double)]
        L.rtw_world_rebuild_tables_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_size_t, C.c_float * 2, C.c_double * 6, C.c_uint32 * 4]
        L.rtw_world_rebuild_refit_tables_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_size_t, C.c_float * 2,
                                                          C.c_double * 6, C.c_uint32 * 4]
    if hasattr(L, "rtw_temporal_device"):  # temporal accumulation
        for f in (L.rtw_temporal_device, L.rtw_temporal_host):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, P(Camera), P(Camera), C.c_void_p, C.c_uint32, C.c_uint32,
                          P(TemporalOpts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rtw_pixel_rays_device.argtypes = [P(Camera), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rtw_world_prev_points_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p]
        L.rtw_world_prev_points_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]
    if hasattr(L, "rtw_temporal_clamped_device"):  # the history clamped to the frame's neighbourhood
        for f in (L.rtw_temporal_clamped_device, L.rtw_temporal_clamped_host):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, P(Camera), P(Camera), C.c_void_p, C.c_uint32, C.c_uint32,
                          P(TemporalOpts), P(TemporalClamp), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "rtw_world_surface_device"):  # surface queries
        for f in (L.rtw_world_surface_device, L.rtw_scene_surface_device):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rtw_world_surface.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    if hasattr(L, "rtw_world_mirror_points_device"):  # mirror points
        L.rtw_world_mirror_points_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, P(Camera), C.c_void_p,
                                                     C.c_void_p, P(MirrorOpts), C.c_void_p, C.c_void_p, C.c_void_p]
        L.rtw_world_mirror_rays_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.rtw_world_mirror_points_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, P(Camera),
                                                   C.c_void_p, C.c_void_p, P(MirrorOpts), C.c_void_p]
    _lib = L
    return L


def header_symbols() -> list[str]:
    """Every function the C ABI header declares (for the export test)."""
    txt = open(HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(rtw_[a-z0-9_]+)\s*\(", txt)))


def _check(status: int):
    if status != RTW_OK:
        raise RtwError(status, (lib().rtw_last_error() or b"").decode())


def abi_version() -> int:
    return lib().rtw_abi_version()


def device_count() -> int:
    return lib().rtw_device_count()


# ------------------------------------------------------ host helpers ----
def camera_init(look_from, look_at, vup, vfov, aspect, aperture, focus_dist, time0=0.0, time1=1.0) -> Camera:
    cam = Camera()
    arr = C.c_double * 3
    _check(lib().rtw_camera_init(C.byref(cam), arr(*look_from), arr(*look_at), arr(*vup), vfov, aspect,
                                 aperture, focus_dist, time0, time1))
    return cam


def cover_camera(aspect: float) -> Camera:
    """Scene-1 camera: main.zig:323-326 and :366-376."""
    return camera_init((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, aspect, 0.1, 10.0, 0.0, 1.0)


def image_height(width: int, aspect: float) -> int:
    return int(lib().rtw_image_height(width, aspect))


def pixel_ray(cam: Camera, width: int, height: int, x: int, y: int) -> Ray:
    """The feature ray of pixel (x, image row y) as the guides define it (rtw_pixel_ray):
    pixel centre, no lens offset, mid-shutter time, t_min 0.001, t_max inf."""
    r = Ray()
    st = lib().rtw_pixel_ray(C.byref(cam), width, height, x, y, C.byref(r))
    if st != RTW_OK:
        raise RtwError(st, f"rtw_pixel_ray: pixel ({x}, {y}) of {width}x{height}")
    return r


def _vp(p):
    return C.c_void_p(p) if p else None


def _surface(entry, handle, hits_ptr, n, surf_ptr, guides_ptr, background, stream):
    """rtw_world_surface_device / rtw_scene_surface_device on device pointers (DeviceWorld.surface,
    DeviceScene.surface)."""
    bg = (C.c_double * 3)(*background) if background is not None else None
    _check(entry(handle, _vp(hits_ptr), n, bg, _vp(surf_ptr), _vp(guides_ptr), _vp(stream)))


def temporal_device(mean_ptr: int, guides_ptr: int, prev_p_ptr: int | None, cam_prev: Camera, cam: Camera,
                    hist_in_ptr: int | None, width: int, height: int, hist_out_ptr: int, mean_out_ptr: int | None = None,
                    var_out_ptr: int | None = None, opts: TemporalOpts | None = None, stream: int | None = None):
    """rtw_temporal_device on device pointers, asynchronous on `stream`: one frame's mean (W*H*3 f32) and
    guides blended into the history image hist_out (W*H rtw_history) from hist_in (None: the first frame);
    prev_p (W*H*3 f64, None: nothing moved) from DeviceWorld.prev_points_device."""
    _check(lib().rtw_temporal_device(_vp(mean_ptr), _vp(guides_ptr), _vp(prev_p_ptr), C.byref(cam_prev), C.byref(cam),
                                     _vp(hist_in_ptr), width, height, C.byref(opts) if opts is not None else None,
                                     _vp(hist_out_ptr), _vp(mean_out_ptr), _vp(var_out_ptr), _vp(stream)))


def temporal_host(mean, guides, cam_prev: Camera, cam: Camera, hist_in=None, prev_p=None,
                  opts: TemporalOpts | None = None):
    """rtw_temporal_host on numpy arrays (no GPU): mean (H, W, 3) float32, guides (H, W) GUIDE_DTYPE, hist_in
    (H, W) HISTORY_DTYPE or None, prev_p (H, W, 3) float64 or None -> (hist_out, mean_out, var_out)."""
    m = np.ascontiguousarray(mean, np.float32)
    g = np.ascontiguousarray(guides, GUIDE_DTYPE)
    H, W = g.shape
    hi = np.ascontiguousarray(hist_in, HISTORY_DTYPE) if hist_in is not None else None
    pp = np.ascontiguousarray(prev_p, np.float64) if prev_p is not None else None
    if m.shape != (H, W, 3) or (hi is not None and hi.shape != (H, W)) or (pp is not None and pp.shape != (H, W, 3)):
        raise ValueError("mean (H, W, 3), guides (H, W), hist_in (H, W), prev_p (H, W, 3)")
    ho, mo, vo = np.zeros((H, W), HISTORY_DTYPE), np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    _check(lib().rtw_temporal_host(m.ctypes.data, g.ctypes.data, pp.ctypes.data if pp is not None else None,
                                   C.byref(cam_prev), C.byref(cam), hi.ctypes.data if hi is not None else None, W, H,
                                   C.byref(opts) if opts is not None else None, ho.ctypes.data, mo.ctypes.data,
                                   vo.ctypes.data, None))
    return ho, mo, vo


def temporal_clamped_device(mean_ptr: int, guides_ptr: int, prev_p_ptr: int | None, cam_prev: Camera, cam: Camera,
                            hist_in_ptr: int | None, width: int, height: int, hist_out_ptr: int,
                            mean_out_ptr: int | None = None, var_out_ptr: int | None = None,
                            opts: TemporalOpts | None = None, clamp: TemporalClamp | None = None,
                            stream: int | None = None):
    """rtw_temporal_clamped_device on device pointers: temporal_device with the history clamped to the window of
    the current mean around each pixel (clamp None: temporal_device's bytes)."""
    _check(lib().rtw_temporal_clamped_device(_vp(mean_ptr), _vp(guides_ptr), _vp(prev_p_ptr), C.byref(cam_prev),
                                             C.byref(cam), _vp(hist_in_ptr), width, height,
                                             C.byref(opts) if opts is not None else None,
                                             C.byref(clamp) if clamp is not None else None, _vp(hist_out_ptr),
                                             _vp(mean_out_ptr), _vp(var_out_ptr), _vp(stream)))


def temporal_clamped_host(mean, guides, cam_prev: Camera, cam: Camera, hist_in=None, prev_p=None,
                          opts: TemporalOpts | None = None, clamp: TemporalClamp | None = None):
    """rtw_temporal_clamped_host on numpy arrays (no GPU): temporal_host's arguments and results, `clamp` after
    `opts` (None: temporal_host's bytes)."""
    m = np.ascontiguousarray(mean, np.float32)
    g = np.ascontiguousarray(guides, GUIDE_DTYPE)
    H, W = g.shape
    hi = np.ascontiguousarray(hist_in, HISTORY_DTYPE) if hist_in is not None else None
    pp = np.ascontiguousarray(prev_p, np.float64) if prev_p is not None else None
    if m.shape != (H, W, 3) or (hi is not None and hi.shape != (H, W)) or (pp is not None and pp.shape != (H, W, 3)):
        raise ValueError("mean (H, W, 3), guides (H, W), hist_in (H, W), prev_p (H, W, 3)")
    ho, mo, vo = np.zeros((H, W), HISTORY_DTYPE), np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    _check(lib().rtw_temporal_clamped_host(m.ctypes.data, g.ctypes.data, pp.ctypes.data if pp is not None else None,
                                           C.byref(cam_prev), C.byref(cam), hi.ctypes.data if hi is not None else None,
                                           W, H, C.byref(opts) if opts is not None else None,
                                           C.byref(clamp) if clamp is not None else None, ho.ctypes.data,
                                           mo.ctypes.data, vo.ctypes.data, None))
    return ho, mo, vo


def pixel_rays_device(cam: Camera, width: int, height: int, rays_ptr: int, stream: int | None = None):
    """rtw_pixel_rays_device: the width*height feature rays (rtw_ray records, row-major) into device memory."""
    _check(lib().rtw_pixel_rays_device(C.byref(cam), width, height, _vp(rays_ptr), _vp(stream)))


def cover_scene(seed: int = 42):
    """generateRandomScene on DefaultPrng.init(seed) -> (spheres, materials, rng_state)."""
    ns, nm = C.c_uint32(0), C.c_uint32(0)
    st = (C.c_uint64 * 4)()
    _check(lib().rtw_cover_scene(seed, None, C.byref(ns), None, C.byref(nm), st))
    sph = (Sphere * ns.value)()
    mats = (Material * nm.value)()
    _check(lib().rtw_cover_scene(seed, sph, C.byref(ns), mats, C.byref(nm), st))
    return sph, mats, [int(x) for x in st]


def make_params(width, height, spp, max_depth=50, seed=42, background=COVER_BACKGROUND, row_begin=0,
                row_stride=1, row_count=None, chunk=0, precision="f64", device=-1, engine="megakernel",
                wf_paths=0, wf_sets=0, wf_drain="samples", wf_form="fused", world_waves=0,
                world_features="auto", world_traversal="auto", wf_bounces=0, wf_passes=0) -> Params:
    """rtw_params (ABI v4): every engine choice is a field (0 / the first
    name = the library default); nothing is read from the environment."""
    if row_count is None:
        row_count = (height - row_begin + row_stride - 1) // row_stride
    prec = PRECISION[precision] if isinstance(precision, str) else int(precision)
    eng = ENGINE[engine] if isinstance(engine, str) else int(engine)

    def enum(v, names):
        return names[v] if isinstance(v, str) else int(v)
    return Params(width, height, spp, max_depth, seed, (C.c_double * 3)(*background), row_begin, row_stride,
                  row_count, chunk, prec, device, eng, wf_paths, wf_sets, enum(wf_drain, WF_DRAIN),
                  enum(wf_form, WF_FORM), world_waves, enum(world_features, WORLD_FEATURES),
                  enum(world_traversal, WORLD_TRAVERSAL), wf_bounces, wf_passes)


def _arr(x, typ):
    if x is None or len(x) == 0:
        return None, 0
    return x, len(x)


def render(cam: Camera, spheres, mats, params: Params, want_mean=False):
    """Synchronous host-buffer render (rtw_render): rgb (rows, W, 3) uint8 [, mean f32]."""
    rgb = np.zeros((params.row_count, params.width, 3), np.uint8)
    mean = np.zeros((params.row_count, params.width, 3), np.float32) if want_mean else None
    s, n = _arr(spheres, Sphere)
    m, nm = _arr(mats, Material)
    _check(lib().rtw_render(C.byref(cam), s, n, m, nm, C.byref(params), rgb.ctypes.data,
                            mean.ctypes.data if want_mean else None))
    return (rgb, mean) if want_mean else rgb


def workspace_bytes(params: Params) -> int:
    n = lib().rtw_workspace_bytes(C.byref(params))
    if n == 0:
        _check(RTW_EINVAL)
    return int(n)


class SclkProbe:
    """Average shader clock (MHz) over a wall-time window (rtw_sclk_probe_*):
    start it on a side stream, run the renders, then read()."""

    def __init__(self, stream: int, wall_ms: float):
        self.h = C.c_void_p()
        _check(lib().rtw_sclk_probe_begin(C.c_void_p(stream), float(wall_ms), C.byref(self.h)))

    def read(self) -> float:
        mhz = C.c_double()
        h, self.h = self.h, C.c_void_p()
        _check(lib().rtw_sclk_probe_end(h, C.byref(mhz)))
        return float(mhz.value)


class Timer:
    """HIP events bracketing the trace kernel on the render stream."""

    def __init__(self):
        self.h = C.c_void_p()
        _check(lib().rtw_timer_create(C.byref(self.h)))

    def elapsed_ms(self) -> float:
        ms = C.c_float()
        _check(lib().rtw_timer_elapsed_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def close(self):
        if self.h:
            lib().rtw_timer_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceScene:
    """A scene resident in HBM of the current device (rtw_scene_create)."""

    def __init__(self, spheres, mats):
        self.h = C.c_void_p()
        s, n = _arr(spheres, Sphere)
        m, nm = _arr(mats, Material)
        _check(lib().rtw_scene_create(s, n, m, nm, C.byref(self.h)))
        self.n_spheres, self.n_materials = n, nm

    def render_async(self, cam: Camera, params: Params, workspace_ptr: int, workspace_bytes_: int,
                     rgb_ptr: int, mean_ptr: int | None = None, stream: int | None = None,
                     timer: Timer | None = None):
        """rtw_render_device on `stream` (a hipStream_t as int) into device buffers."""
        _check(lib().rtw_render_device(self.h, C.byref(cam), C.byref(params), C.c_void_p(workspace_ptr),
                                       workspace_bytes_, C.c_void_p(rgb_ptr),
                                       C.c_void_p(mean_ptr) if mean_ptr else None,
                                       C.c_void_p(stream) if stream else None,
                                       timer.h if timer is not None else None))

    def guides(self, cam: Camera, params: Params, guides_ptr: int, stream: int | None = None):
        """The scene's feature buffers (rtw_scene_guides_device): row_count x W rtw_guide
        records (32 bytes each) into device memory, asynchronous on `stream`."""
        _check(lib().rtw_scene_guides_device(self.h, C.byref(cam), C.byref(params), C.c_void_p(guides_ptr),
                                             C.c_void_p(stream) if stream else None))

    def trace(self, rays_ptr: int, n: int, hits_ptr: int, stream: int | None = None):
        """Closest hits of n rtw_ray records in device memory into n rtw_hit records
        (rtw_scene_trace_device), asynchronous on `stream`; prim = sphere index + 1."""
        _check(lib().rtw_scene_trace_device(self.h, C.c_void_p(rays_ptr), n, C.c_void_p(hits_ptr),
                                            C.c_void_p(stream) if stream else None))

    def occluded(self, rays_ptr: int, n: int, out_ptr: int, stream: int | None = None):
        """One byte per ray, 1 where trace() would hit (rtw_scene_occluded_device)."""
        _check(lib().rtw_scene_occluded_device(self.h, C.c_void_p(rays_ptr), n, C.c_void_p(out_ptr),
                                               C.c_void_p(stream) if stream else None))

    def trace_host(self, rays) -> np.ndarray:
        """rtw_scene_trace: rays (n,) RAY_DTYPE on the host -> hits (n,) HIT_DTYPE, synchronous."""
        r = np.ascontiguousarray(rays, RAY_DTYPE)
        out = np.zeros(r.shape, HIT_DTYPE)
        _check(lib().rtw_scene_trace(self.h, r.ctypes.data, r.size, out.ctypes.data))
        return out

    def surface(self, hits_ptr: int, n: int, surf_ptr: int | None = None, guides_ptr: int | None = None,
                background=None, stream: int | None = None):
        """rtw_scene_surface_device: for n rtw_hit records of this scene in device memory, n rtw_surface
        records (64 bytes each) and / or n rtw_guide records, asynchronous on `stream`; the materials are
        reported in the world's enumerations.  `background` (three numbers) is needed with guides_ptr."""
        _surface(lib().rtw_scene_surface_device, self.h, hits_ptr, n, surf_ptr, guides_ptr, background, stream)

    def counts(self, cam: Camera, params: Params, workspace_ptr: int, workspace_bytes_: int) -> dict:
        out = (C.c_uint64 * 6)()
        _check(lib().rtw_render_counts_ex(self.h, C.byref(cam), C.byref(params), C.c_void_p(workspace_ptr),
                                          workspace_bytes_, out))
        return {"samples": int(out[0]), "segments": int(out[1]), "static_tests": int(out[2]),
                "moving_tests": int(out[3]), "drain_segments": int(out[4]), "drain_samples": int(out[5])}

    def stats(self, cam: Camera, params: Params, workspace_ptr: int, workspace_bytes_: int) -> dict:
        """The counting pass's raw statistics words (rtw_render_stats, RTW_STAT_*)."""
        if hasattr(lib(), "rtw_render_stats_ex"):
            n = len(STAT_NAMES_EX) + STATS_WORDS - len(STAT_NAMES)  # (words 14-15 of the 16 are named since round 11)
            out = (C.c_uint64 * n)()
            _check(lib().rtw_render_stats_ex(self.h, C.byref(cam), C.byref(params), C.c_void_p(workspace_ptr),
                                             workspace_bytes_, out, n))
            names = STAT_NAMES + [None] * (STATS_WORDS - len(STAT_NAMES)) + STAT_NAMES_EX[len(STAT_NAMES):]
            return {k: int(out[i]) for i, k in enumerate(names) if k}
        out = (C.c_uint64 * STATS_WORDS)()
        _check(lib().rtw_render_stats(self.h, C.byref(cam), C.byref(params), C.c_void_p(workspace_ptr),
                                      workspace_bytes_, out))
        return {n: int(out[i]) for i, n in enumerate(STAT_NAMES)}

    def close(self):
        if self.h:
            lib().rtw_scene_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def denoise_workspace_bytes(width: int, height: int, opts: DenoiseOpts | None = None) -> int:
    n = lib().rtw_denoise_workspace_bytes(width, height, C.byref(opts) if opts is not None else None)
    if n == 0:
        _check(RTW_EINVAL)
    return int(n)


def denoise_host(mean, var=None, guides=None, opts: DenoiseOpts | None = None):
    """The denoiser on the CPU (rtw_denoise_host; needs no GPU): mean (H, W, 3)
    f32, var (H, W) f32 or None, guides (H, W) GUIDE_DTYPE or None ->
    (rgb (H, W, 3) uint8, mean (H, W, 3) f32).  The device entries give these bytes."""
    m = np.ascontiguousarray(mean, np.float32)
    h, w = m.shape[:2]
    v = None if var is None else np.ascontiguousarray(var, np.float32)
    g = None if guides is None else np.ascontiguousarray(guides, GUIDE_DTYPE)
    if (v is not None and v.size != h * w) or (g is not None and g.size != h * w):
        raise ValueError("var / guides do not have the image's size")
    nbytes = denoise_workspace_bytes(w, h, opts)
    ws = np.empty(nbytes // 16 + 1, np.dtype([("p", np.float32, 4)]))  # (16-byte records; numpy aligns to 16)
    ptr = (ws.ctypes.data + 15) & ~15
    rgb, out = np.empty((h, w, 3), np.uint8), np.empty((h, w, 3), np.float32)
    _check(lib().rtw_denoise_host(m.ctypes.data, v.ctypes.data if v is not None else None,
                                  g.ctypes.data if g is not None else None, w, h,
                                  C.byref(opts) if opts is not None else None, C.c_void_p(ptr),
                                  ws.nbytes - (ptr - ws.ctypes.data), rgb.ctypes.data, out.ctypes.data, None))
    return rgb, out


def denoise_device(mean_ptr: int, var_ptr: int | None, guides_ptr: int | None, width: int, height: int,
                   opts: DenoiseOpts | None, workspace_ptr: int, workspace_bytes_: int, rgb_ptr: int | None,
                   mean_out_ptr: int | None, stream: int | None = None):
    """rtw_denoise_device on plain device buffers, asynchronous on `stream`."""
    def vp(x):
        return C.c_void_p(x) if x else None
    _check(lib().rtw_denoise_device(vp(mean_ptr), vp(var_ptr), vp(guides_ptr), width, height,
                                    C.byref(opts) if opts is not None else None, vp(workspace_ptr), workspace_bytes_,
                                    vp(rgb_ptr), vp(mean_out_ptr), vp(stream)))


def spatial_variance_host(mean, var=None, guides=None, opts: DenoiseOpts | None = None):
    """The spatial variance estimate on the CPU (rtw_denoise_spatial_variance_host;
    needs no GPU): mean (H, W, 3) f32, var (H, W) f32 or None (all unknown),
    guides (H, W) GUIDE_DTYPE or None -> var (H, W) f32 with every VAR_UNKNOWN
    pixel replaced by the guide-weighted variance of its 7x7 window's luminance.
    denoise_host with DENOISE_SPATIAL_VAR is denoise_host on this map."""
    m = np.ascontiguousarray(mean, np.float32)
    h, w = m.shape[:2]
    v = None if var is None else np.ascontiguousarray(var, np.float32)
    g = None if guides is None else np.ascontiguousarray(guides, GUIDE_DTYPE)
    if (v is not None and v.size != h * w) or (g is not None and g.size != h * w):
        raise ValueError("var / guides do not have the image's size")
    out = np.empty((h, w), np.float32)
    _check(lib().rtw_denoise_spatial_variance_host(m.ctypes.data, v.ctypes.data if v is not None else None,
                                                   g.ctypes.data if g is not None else None, w, h,
                                                   C.byref(opts) if opts is not None else None, out.ctypes.data, None))
    return out


def spatial_variance_device(mean_ptr: int, var_ptr: int | None, guides_ptr: int | None, width: int, height: int,
                            opts: DenoiseOpts | None, var_out_ptr: int, stream: int | None = None):
    """rtw_denoise_spatial_variance_device on plain device buffers, asynchronous on `stream`."""
    def vp(x):
        return C.c_void_p(x) if x else None
    _check(lib().rtw_denoise_spatial_variance_device(vp(mean_ptr), vp(var_ptr), vp(guides_ptr), width, height,
                                                     C.byref(opts) if opts is not None else None, vp(var_out_ptr),
                                                     vp(stream)))


def effective_chunk(params: Params) -> int:
    """The accumulation chunk a render of `params` uses (rtw_hip.h)."""
    return min(params.chunk or DEFAULT_CHUNK, params.spp)


class Accumulator:
    """A frame accumulated over sample passes (rtw_accum_*): render some
    samples, resolve the image, render more; read() / load() save and resume.
    `target` is a DeviceScene (cover-scene engines) or a world.DeviceWorld.
    After passes totalling N samples (a multiple of the chunk, or params.spp)
    the resolved image is the one-shot render's with spp = N, byte for byte.
    Passes, resolves and noise queries go on one stream.

    Adaptive sampling (rtw_hip.h): set_mask() / set_adaptive()
    put the accumulator in the masked state, where it keeps per-pixel sample
    counts (counts()) and an active set (active()).  A pass then renders the
    active pixels only, a pixel that went inactive stays so, and a pixel with
    count n holds the one-shot render's bytes with spp = n at that pixel.  In
    that state render_pass() first waits on the host for the previous pass's
    active-tile count (one small readback per pass); with no active pixel it
    does nothing.  Masked passes save time, not workspace."""

    def __init__(self, target, params: Params):
        self.target = target
        self.params = params
        self.is_world = not isinstance(target, DeviceScene)
        self.chunk = effective_chunk(params)
        self.npix = params.row_count * params.width
        self.h = C.c_void_p()
        self.masked = False  # set_mask / set_adaptive(tol > 0) / load(counts=) called: per-pixel counts, active set
        _check(lib().rtw_accum_create(C.byref(params), C.byref(self.h)))

    def workspace_bytes(self, pass_spp: int) -> int:
        """Device workspace of a pass of pass_spp samples.  A last pass shorter
        than the chunk's next multiple is sized as that multiple."""
        n = min(max(1, -(-pass_spp // self.chunk)) * self.chunk, self.params.spp)
        if self.is_world:
            b = lib().rtw_accum_world_workspace_bytes(self.target.h, C.byref(self.params), n)
        else:
            b = lib().rtw_accum_workspace_bytes(C.byref(self.params), n)
        if b == 0:
            _check(RTW_EINVAL)
        return int(b)

    def render_pass(self, cam: Camera, pass_spp: int, workspace_ptr: int, workspace_bytes_: int,
                    stream: int | None = None, timer: Timer | None = None):
        """One pass of pass_spp samples, asynchronous on `stream` (a hipStream_t as int)."""
        f = lib().rtw_accum_world_render_device if self.is_world else lib().rtw_accum_render_device
        _check(f(self.h, self.target.h, C.byref(cam), pass_spp, C.c_void_p(workspace_ptr), workspace_bytes_,
                 C.c_void_p(stream) if stream else None, timer.h if timer is not None else None))

    def resolve(self, rgb_ptr: int, mean_ptr: int | None = None, stream: int | None = None):
        """The image of the samples so far into device buffers (rtw_accum_resolve_device)."""
        _check(lib().rtw_accum_resolve_device(self.h, C.c_void_p(rgb_ptr), C.c_void_p(mean_ptr) if mean_ptr else None,
                                              C.c_void_p(stream) if stream else None))

    def variance(self, var_ptr: int, stream: int | None = None):
        """Per-pixel variance of the mean luminance, (rows, W) f32 into device memory
        (rtw_accum_variance_device): VAR_UNKNOWN below two full chunks, VAR_EMPTY without a sample."""
        _check(lib().rtw_accum_variance_device(self.h, C.c_void_p(var_ptr), C.c_void_p(stream) if stream else None))

    def denoise_workspace_bytes(self, opts: DenoiseOpts | None = None) -> int:
        n = lib().rtw_accum_denoise_workspace_bytes(self.h, C.byref(opts) if opts is not None else None)
        if n == 0:
            _check(RTW_EINVAL)
        return int(n)

    def denoise(self, guides_ptr: int | None, workspace_ptr: int, workspace_bytes_: int, rgb_ptr: int | None,
                mean_ptr: int | None = None, opts: DenoiseOpts | None = None, stream: int | None = None):
        """The denoised image of the samples so far (rtw_accum_denoise_device: resolve,
        variance, filter) into device buffers.  The accumulator is not modified.
        opts.flags DENOISE_SPATIAL_VAR: pixels below two full chunks — every pixel of a
        first single-chunk pass — get their variance estimated from the image."""
        def vp(x):
            return C.c_void_p(x) if x else None
        _check(lib().rtw_accum_denoise_device(self.h, vp(guides_ptr), C.byref(opts) if opts is not None else None,
                                              vp(workspace_ptr), workspace_bytes_, vp(rgb_ptr), vp(mean_ptr),
                                              vp(stream)))

    def samples(self) -> int:
        n = C.c_uint32()
        _check(lib().rtw_accum_samples(self.h, C.byref(n)))
        return int(n.value)

    def noise(self, stream: int | None = None) -> float:
        """RMS standard error of the pixels' mean luminance (synchronous)."""
        x = C.c_double()
        _check(lib().rtw_accum_noise(self.h, C.c_void_p(stream) if stream else None, C.byref(x)))
        return float(x.value)

    def read(self):
        """(sum (rows, W, 3) f64, stat (rows, W, 2) f64) on the host (synchronous)."""
        shape = (self.params.row_count, self.params.width)
        s, t = np.empty(shape + (3,), np.float64), np.empty(shape + (2,), np.float64)
        _check(lib().rtw_accum_read(self.h, s.ctypes.data, t.ctypes.data))
        return s, t

    def load(self, sum_, stat, samples_done: int, counts=None):
        """Replace the state with a saved one (rtw_accum_load; with `counts`,
        the per-pixel sample counts of counts(): rtw_accum_load_counts)."""
        s = np.ascontiguousarray(sum_, np.float64)
        t = np.ascontiguousarray(stat, np.float64)
        if s.size != self.npix * 3 or t.size != self.npix * 2:
            raise ValueError("sum / stat do not have this accumulator's size")
        if counts is None:
            _check(lib().rtw_accum_load(self.h, s.ctypes.data, t.ctypes.data, samples_done))
            return
        c = np.ascontiguousarray(counts, np.uint32)
        if c.size != self.npix:
            raise ValueError("counts do not have this accumulator's size")
        _check(lib().rtw_accum_load_counts(self.h, s.ctypes.data, t.ctypes.data, c.ctypes.data, samples_done))
        self.masked = True

    def set_mask(self, mask):
        """active &= (mask != 0); mask: (rows, W), any integer or bool type (synchronous)."""
        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        if m.size != self.npix:
            raise ValueError("mask does not have this accumulator's size")
        _check(lib().rtw_accum_set_mask(self.h, m.ctypes.data))
        self.masked = True

    def set_adaptive(self, tol: float, min_spp: int = 0):
        """Per-pixel noise budget: a pixel stops once the standard error of its
        mean luminance is <= tol (absolute) and it holds >= min_spp samples;
        tol = 0 removes the budget (rtw_accum_set_adaptive)."""
        _check(lib().rtw_accum_set_adaptive(self.h, float(tol), int(min_spp)))
        self.masked = self.masked or tol > 0

    def active(self):
        """(active pixels, tiles that hold one) (synchronous)."""
        a, b = C.c_uint32(), C.c_uint32()
        _check(lib().rtw_accum_active(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def counts(self):
        """Per-pixel sample counts, (rows, W) uint32 on the host (synchronous)."""
        c = np.empty((self.params.row_count, self.params.width), np.uint32)
        _check(lib().rtw_accum_read_counts(self.h, c.ctypes.data))
        return c

    def close(self):
        if self.h:
            lib().rtw_accum_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
