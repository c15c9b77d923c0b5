/*
 * rtw_hip.h — C ABI of the MI355X (gfx950) path tracer for the RTIOW cover
 * scene.  Drop-in for the render loop of nsfisis/RayTracingInOneWeekend.zig.
 *
 * The reference has no plugin/FFI surface for this path: Camera, rayColor and
 * the render loop are private to src/main.zig (Camera: main.zig:40-101,
 * rayColor: main.zig:103-122, loop: main.zig:378-402).  This header defines
 * the boundary a Zig host would bind with `extern "rtw_hip" fn ...` (see
 * INTEGRATION.md): the host keeps building the world with the src/rtw API
 * (Hittable / Material / Texture) and flattens it into the plain arrays below.
 *
 * Conventions: plain C types only; 0 = success, negative = rtw_status;
 * the message of the last failure on the calling thread is rtw_last_error().
 * No pointer passed in is retained after a call returns (except device
 * buffers used by a still-running async render on the caller's stream).
 */
#ifndef RTW_HIP_H
#define RTW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTW_ABI_VERSION 4

typedef enum {
  RTW_OK = 0,
  RTW_EINVAL = -1,      /* bad argument (null pointer, zero size, out of range) */
  RTW_UNSUPPORTED = -2, /* primitive / material / size the kernel does not implement */
  RTW_EHIP = -3,        /* HIP runtime error (message has the HIP error string) */
  RTW_ENOMEM = -4,      /* device allocation failed */
  RTW_ENODEV = -5       /* no GPU visible */
} rtw_status;

/* Material kinds: Material union (material.zig:16-21) x Texture union
 * (texture.zig:10-14) flattened.  DiffuseLight / noise / image textures are
 * not in the cover scene and return RTW_UNSUPPORTED. */
typedef enum {
  RTW_LAMBERT_SOLID = 0,   /* DiffuseMaterial{SolidTexture}   material.zig:41-53, texture.zig:46-55 */
  RTW_LAMBERT_CHECKER = 1, /* DiffuseMaterial{CheckerTexture} texture.zig:57-83 */
  RTW_METAL = 2,           /* MetalMaterial                   material.zig:55-66 */
  RTW_DIELECTRIC = 3,      /* DielectricMaterial              material.zig:68-92 */
  RTW_DIFFUSE_LIGHT = 4    /* DiffuseLightMaterial            material.zig:94-110 (unsupported) */
} rtw_material_kind;

typedef struct {
  uint32_t kind;          /* rtw_material_kind */
  uint32_t reserved;
  double albedo[3];       /* solid colour; checker EVEN colour; metal albedo */
  double albedo_odd[3];   /* checker ODD colour (texture.zig:79-82) */
  double fuzz;            /* metal fuzz (<= 1, material.zig:60) */
  double ir;              /* dielectric index of refraction */
} rtw_material;

/* Sphere (hittable.zig:90-94) or MovingSphere (hittable.zig:157-164). */
typedef struct {
  double c0[3];           /* center / center0 */
  double c1[3];           /* center1 (== c0 for a static sphere) */
  double radius;
  double t0, t1;          /* MovingSphere time0 / time1 (ignored when !moving) */
  uint32_t moving;        /* 0 = Sphere, 1 = MovingSphere */
  uint32_t mat;           /* index into the material array */
} rtw_sphere;

/* Camera fields (main.zig:40-50), computed on the host in f64 by
 * rtw_camera_init (= Camera.init, main.zig:52-89). */
typedef struct {
  double origin[3], horizontal[3], vertical[3], lower_left_corner[3];
  double u[3], v[3], w[3];
  double lens_radius, time0, time1;
} rtw_camera;

typedef enum {
  RTW_PRECISION_F64 = 0,      /* the reference's arithmetic (f64 everywhere) */
  RTW_PRECISION_F32 = 1       /* f32 + f64 for radius >= 100 spheres + convex self-skip */
} rtw_precision;

/* Render engine (both compute the same Tier-B image, bit for bit). */
typedef enum {
  RTW_ENGINE_MEGAKERNEL = 0,  /* one persistent trace kernel (BASELINE.json configs[1]) */
  RTW_ENGINE_WAVEFRONT = 1    /* per-bounce kernels over SoA path queues in HBM (configs[3]) */
} rtw_engine;

/* Wavefront engine, once the unit queue runs dry.  Every
 * choice renders the same image, bit for bit. */
typedef enum {
  RTW_WF_DRAIN_SAMPLES = 0,   /* wf_drain: a segment's remaining samples dealt to its free lanes (default) */
  RTW_WF_DRAIN_SLOTS = 1,     /* wf_finish: each lane runs its own slot's remaining samples */
  RTW_WF_DRAIN_NONE = 2       /* no in-register drain: the bounce kernels' queues run to the end */
} rtw_wf_drain;
typedef enum {
  RTW_WF_FUSED = 0,           /* one kernel per bounce: shade + the next closest hit (default) */
  RTW_WF_SPLIT = 1            /* separate extend (closest hit) and shade kernels per bounce */
} rtw_wf_form;

/* World kernel instantiation (rtw_world_*; every choice gives the same bits). */
typedef enum {
  RTW_WORLD_FEATURES_AUTO = 0, /* the smallest compiled feature set holding the world's features */
  RTW_WORLD_FEATURES_ALL = 1   /* the general kernel (every primitive, texture and transform) */
} rtw_world_features;
typedef enum {
  RTW_WORLD_TRAVERSAL_AUTO = 0,  /* per lane for sphere worlds of >= 256 BVH nodes, else the union */
  RTW_WORLD_TRAVERSAL_UNION = 1, /* the wave walks the union of its lanes' BVH paths (scalar node loads) */
  RTW_WORLD_TRAVERSAL_LANE = 2,  /* every lane walks its own path (sphere worlds with a BVH of depth <= 16 —
                                    rtw_world_create caps the depth of large sphere worlds' trees at 16 —
                                    other worlds take the union walk) */
  RTW_WORLD_TRAVERSAL_LINEAR = 3 /* (reported only, rtw_world_launch_info: a world without a BVH) */
} rtw_world_traversal;

typedef struct {
  uint32_t width, height;     /* full image (main.zig:305-306) */
  uint32_t spp;               /* samples_per_pixel (main.zig:308) */
  uint32_t max_depth;         /* max_depth (main.zig:307), 50 in the reference */
  uint64_t seed;              /* RNG seed (main.zig:300 uses 42) */
  double background[3];       /* main.zig:322 */
  uint32_t row_begin;         /* first IMAGE row rendered (top-first, main.zig:396) */
  uint32_t row_stride;        /* image-row stride (row sharding across GPUs) */
  uint32_t row_count;         /* rows rendered; output row q = image row row_begin+q*row_stride */
  uint32_t chunk;             /* samples per accumulation chunk, 0 = default (RTW_DEFAULT_CHUNK) */
  uint32_t precision;         /* rtw_precision */
  int32_t device;             /* HIP device for rtw_render (-1 = current) */
  uint32_t engine;            /* rtw_engine */
  uint32_t wf_paths;          /* wavefront: in-flight paths (queue capacity), 0 = RTW_DEFAULT_WF_PATHS */
  /* ABI v4: engine configuration, all 0 = default.  The library reads no
   * environment variable on the render path; rtw_workspace_bytes depends on
   * these fields only. */
  uint32_t wf_sets;           /* wavefront: independent queue sets (1-4), 0 = RTW_DEFAULT_WF_SETS */
  uint32_t wf_drain;          /* wavefront: rtw_wf_drain */
  uint32_t wf_form;           /* wavefront: rtw_wf_form */
  uint32_t world_waves;       /* world kernel: register budget in waves per SIMD: 3 or 4, or 1 = unconstrained
                                 (any other value fails with RTW_EINVAL); 0 = the feature set's default
                                 (4 sphere worlds, 3 rects / transforms, 1 noise textures) */
  uint32_t world_features;    /* world kernel: rtw_world_features */
  uint32_t world_traversal;   /* world kernel: rtw_world_traversal */
  uint32_t wf_bounces;        /* wavefront: bounce segments per path per wf_step launch (the path stays in
                                 registers between them), 0 = 1: one queue exchange per bounce (configs[3]) */
  uint32_t wf_passes;         /* wavefront, fused form: queue passes per wf_step launch (every pass moves each
                                 path through the queues), 0 = RTW_DEFAULT_WF_PASSES; at most 64.  (Round 5,
                                 in the place of v4's `reserved`: same layout, and 0 keeps the default.) */
} rtw_params;

/* Samples per accumulation chunk (a work unit = one pixel x one chunk; the
 * image's per-pixel sum adds each chunk's samples in order, then the chunks in
 * order: DESIGN.md §2).  Round 6: 20 (was 32) — every engine equal or faster,
 * the world kernel 3-10 % (profiles/r06/chunk_ab.txt); 20 divides every
 * configured spp (100, 200, 500, 2000). */
#define RTW_DEFAULT_CHUNK 20u
#define RTW_DEFAULT_WF_PATHS (5u << 17) /* 655,360 in-flight paths (with two sets; round 6) */
/* Wavefront queue sets: wf_paths is split over this many independent queue
 * sets, each driven on its own HIP stream (params.wf_sets overrides, 1-4). */
#define RTW_DEFAULT_WF_SETS 2u
#define RTW_MAX_WF_SETS 4u
/* Queue passes per wf_step launch (round 6: 16 with the paths above). */
#define RTW_DEFAULT_WF_PASSES 16u
#define RTW_MAX_SPHERES 4096u

/* ------------------------------------------------------------ queries -- */
int rtw_abi_version(void);
int rtw_device_count(void);
const char *rtw_last_error(void);

/* ------------------------------------------------- host-side helpers --- */
/* Camera.init (main.zig:52-89).  vfov in degrees. */
int rtw_camera_init(rtw_camera *cam, const double look_from[3], const double look_at[3],
                    const double vup[3], double vfov, double aspect_ratio, double aperture,
                    double focus_dist, double time0, double time1);
/* image_height = @intFromFloat(@divTrunc(@as(f64, width), aspect)) (main.zig:306). */
uint32_t rtw_image_height(uint32_t width, double aspect_ratio);
/* generateRandomScene (main.zig:157-221) on DefaultPrng.init(seed)
 * (main.zig:300).  Writes at most *n_spheres / *n_mats entries (in: capacity,
 * out: count).  rng_state_out (optional): the Xoshiro256 state after the
 * build, i.e. where the reference's render loop continues the stream. */
int rtw_cover_scene(uint64_t seed, rtw_sphere *spheres, uint32_t *n_spheres,
                    rtw_material *mats, uint32_t *n_mats, uint64_t rng_state_out[4]);

/* ------------------------------------------------------------ render --- */
/* Replaces the render loop main.zig:378-402.  Host buffers, synchronous.
 * rgb_out:  W * row_count * 3 bytes, rows in output order (see rtw_params).
 * mean_out: optional, W * row_count * 3 floats = pixel sum / spp (linear). */
int rtw_render(const rtw_camera *cam, const rtw_sphere *spheres, uint32_t n_spheres,
               const rtw_material *mats, uint32_t n_mats, const rtw_params *params,
               uint8_t *rgb_out, float *mean_out);

/* ---------------------------------------------- device-resident API --- */
typedef struct rtw_scene_s *rtw_scene;

/* Upload (validate + flatten) a scene to the CURRENT HIP device. */
int rtw_scene_create(const rtw_sphere *spheres, uint32_t n_spheres, const rtw_material *mats,
                     uint32_t n_mats, rtw_scene *out);
int rtw_scene_destroy(rtw_scene scene);

/* Device workspace needed by rtw_render_device for these params. */
size_t rtw_workspace_bytes(const rtw_params *params);

/* Optional kernel timer around the trace kernel (HIP events on the stream). */
typedef struct rtw_timer_s *rtw_timer;
int rtw_timer_create(rtw_timer *out);
int rtw_timer_destroy(rtw_timer t);
int rtw_timer_elapsed_ms(rtw_timer t, float *ms); /* waits for the stop event */

/* Shader-clock probe (diagnostic, for the bench line): one wave on `stream`
 * (launch it on a stream other than the render's) spins for `wall_ms` of wall
 * time and measures the SIMD clock over that window as
 * delta(s_memtime) / delta(s_memrealtime) x 100 MHz — the average SCLK while
 * the renders launched meanwhile run.  _end waits for the probe and frees it. */
typedef struct rtw_sclk_probe_s *rtw_sclk_probe;
int rtw_sclk_probe_begin(void *stream, double wall_ms, rtw_sclk_probe *out);
int rtw_sclk_probe_end(rtw_sclk_probe p, double *mhz);

/* Asynchronous render on `stream` (hipStream_t, NULL = default stream) into
 * DEVICE buffers d_rgb (W*row_count*3 bytes) and optional d_mean
 * (W*row_count*3 floats).  workspace: >= rtw_workspace_bytes(params) bytes
 * of device memory, 256-byte aligned.  timer (optional) brackets the trace
 * kernel.  Megakernel engine: graph-capturable (no allocation, no
 * synchronisation).  Wavefront engine: the host polls the queue length
 * between batches of bounce kernels, so the call returns after the last
 * bounce kernel was ENQUEUED (the finalize kernel is still asynchronous) and
 * it cannot be captured into a graph; the timer brackets all its kernels. */
int rtw_render_device(rtw_scene scene, const rtw_camera *cam, const rtw_params *params,
                      void *workspace, size_t workspace_bytes, uint8_t *d_rgb, float *d_mean,
                      void *stream, rtw_timer timer);

/* Statistics pass (diagnostic, not the product path's timing): counts the
 * bounce segments and sphere tests the same render performs.  counts_out[4] =
 * {samples, segments, static_tests, moving_tests}. Synchronous.  Both engines
 * count samples and segments (the wavefront engine in its shading step). */
int rtw_render_counts(rtw_scene scene, const rtw_camera *cam, const rtw_params *params,
                      void *workspace, size_t workspace_bytes, uint64_t counts_out[4]);
/* The same pass with counts_out[6]: the four above, then the segments traced
 * and the samples finished by the wavefront engine's in-register drain
 * (paths that no longer stream through the HBM queues; 0 for the megakernel
 * and with RTW_WF_DRAIN_NONE). */
int rtw_render_counts_ex(rtw_scene scene, const rtw_camera *cam, const rtw_params *params,
                         void *workspace, size_t workspace_bytes, uint64_t counts_out[6]);
/* The same pass with the kernels' raw statistics words (diagnostic):
 * stats_out[RTW_STATS_WORDS], indices RTW_STAT_*. */
#define RTW_STATS_WORDS 16
enum {
  RTW_STAT_SAMPLES = 0, RTW_STAT_SEGMENTS = 1, RTW_STAT_F32_SKIPS = 2,
  RTW_STAT_CAND_WAVE_ITERS = 3, RTW_STAT_CAND_LANES = 4, RTW_STAT_DISC_GE0_LANES = 5,
  RTW_STAT_SPHERE_LOOP_WAVE_ITERS = 6, RTW_STAT_CULL_SURVIVOR_LANES = 7, RTW_STAT_CULL_EXACT_WAVE_ITERS = 8,
  RTW_STAT_DRAIN_SEGMENTS = 9, RTW_STAT_DRAIN_SAMPLES = 10, RTW_STAT_CLUSTER_WAVE_TESTS = 11,
  RTW_STAT_CLUSTER_WAVE_SKIPS = 12, RTW_STAT_DRAIN_WAVE_ITERS = 13,
  /* megakernel, primary-first loop: wave-iterations with a primary phase; lanes whose sample ended in
   * it (a camera ray that missed, or max_depth 0) and sat out the rest of that iteration */
  RTW_STAT_PRIMARY_ROUNDS = 14, RTW_STAT_PRIMARY_IDLE_LANES = 15
};
int rtw_render_stats(rtw_scene scene, const rtw_camera *cam, const rtw_params *params,
                     void *workspace, size_t workspace_bytes, uint64_t stats_out[RTW_STATS_WORDS]);
/* The same pass with the first n_words <= RTW_STATS_WORDS_EX words: the RTW_STAT_* ones, then the
 * words added since (additive: rtw_render_stats keeps its 16). */
#define RTW_STATS_WORDS_EX 24
enum {
  /* megakernel, primary-first loop: the fetched unit batches' tile masks, their popcounts summed
   * (spheres the batch's camera rays are tested against per lane) */
  RTW_STAT_PRIMARY_MASK_POPCOUNT = 16,
  /* megakernel, primary-first loop, after a wave's unit queue ran dry (its tail): samples a lane traced
   * for another lane's unit; wave-iterations run in that state; lane-slots of those iterations with no
   * sample in flight or to start, the lane's own or another lane's.  The last two are counted whether
   * or not the launch hands samples out. */
  RTW_STAT_TAIL_HELPED_SAMPLES = 17, RTW_STAT_TAIL_WAVE_ITERS = 18, RTW_STAT_TAIL_IDLE_LANE_ITERS = 19,
  /* megakernel, primary-first loop: units, and their samples, finished without tracing because no camera
   * ray of their tile can hit a sphere (each sample adds the background once; counted in SAMPLES and
   * SEGMENTS as a traced miss is, in no other word) */
  RTW_STAT_UNTRACED_UNITS = 20, RTW_STAT_UNTRACED_SAMPLES = 21,
  /* megakernel, primary-first loop: atomics issued on the launch's unit queue (a claim takes one or
   * several 64-unit batches; the count varies from run to run), and beam passes made (a fetched batch of
   * the tile of the wave's last pass reuses it; PRIMARY_MASK_POPCOUNT stays per fetched batch) */
  RTW_STAT_QUEUE_CLAIMS = 22, RTW_STAT_BEAM_PASSES = 23
};
int rtw_render_stats_ex(rtw_scene scene, const rtw_camera *cam, const rtw_params *params,
                        void *workspace, size_t workspace_bytes, uint64_t *stats_out, uint32_t n_words);

/* =================================================== general worlds ===
 * Every other scene of the reference (main.zig:123-290) and BASELINE.json
 * configs[4] (globe + 10k spheres): the full Hittable / Material / Texture
 * vocabulary, flattened.  Nested lists (Box = 6 rects) become consecutive
 * primitives in list order; Translate / RotateY wrappers become a transform
 * chain per primitive.  Rendered by the world kernel (f64, BVH traversal),
 * whose per-sample contract is oracle/rtw_world.h Tier B. */

typedef enum {
  RTW_PRIM_SPHERE = 0,        /* Sphere        hittable.zig:90-155  a = c[3], c[3], r, 0, 0 */
  RTW_PRIM_MOVING_SPHERE = 1, /* MovingSphere  hittable.zig:157-226 a = c0[3], c1[3], r, t0, t1 */
  RTW_PRIM_XY_RECT = 2,       /* XyRect        hittable.zig:270-323 a = x0, x1, y0, y1, k */
  RTW_PRIM_XZ_RECT = 3,       /* XzRect        hittable.zig:325-378 a = x0, x1, z0, z1, k */
  RTW_PRIM_YZ_RECT = 4,       /* YzRect        hittable.zig:380-427 a = y0, y1, z0, z1, k */
  /* Not in the reference (arithmetic: csrc/rtw_tri.hpp).  rtw_hit.u, v = the barycentric
   * weights of v1 and v2; front when n . d < 0 with n = unit((v1 - v0) x (v2 - v0)); the normal faces the
   * ray.  A non-finite vertex or zero area: RTW_EINVAL at creation, update and rebuild (the world is left
   * untouched).  rtw_world_prev_points_* and rtw_world_mirror_points_* return RTW_UNSUPPORTED for a world
   * or description that holds one. */
  RTW_PRIM_TRIANGLE = 5       /* a = v0[3], v1[3], v2[3] */
} rtw_prim_kind;

typedef struct {
  uint32_t kind, mat;
  int32_t xform;              /* index into xforms, -1 = none */
  uint32_t reserved;
  double a[9];
} rtw_prim;

#define RTW_MAX_XFORM_OPS 4
typedef enum {
  RTW_XF_TRANSLATE = 0,       /* Translate hittable.zig:472-503: v = offset */
  RTW_XF_ROTATE_Y = 1         /* RotateY   hittable.zig:505-608: v = {sin_t, cos_t, angle} */
} rtw_xform_op;
typedef struct {              /* op[0] is the OUTERMOST wrapper */
  uint32_t n;
  uint32_t op[RTW_MAX_XFORM_OPS];
  double v[RTW_MAX_XFORM_OPS][3];
} rtw_xform;

typedef enum {
  RTW_TEX_SOLID = 0,          /* texture.zig:46-55 */
  RTW_TEX_CHECKER = 1,        /* texture.zig:57-83 (solid odd / even) */
  RTW_TEX_NOISE = 2,          /* texture.zig:85-105 (perlin index, scale) */
  RTW_TEX_IMAGE = 3           /* texture.zig:107-144 (image index) */
} rtw_texture_kind;
typedef struct {
  uint32_t kind, perlin, image, reserved;
  double color[3], odd[3], even[3];
  double scale;
} rtw_texture;

typedef enum {
  RTW_WMAT_LAMBERT = 0,       /* DiffuseMaterial      material.zig:41-53 (albedo texture) */
  RTW_WMAT_METAL = 1,         /* MetalMaterial        material.zig:55-66 */
  RTW_WMAT_DIELECTRIC = 2,    /* DielectricMaterial   material.zig:68-92 */
  RTW_WMAT_LIGHT = 3          /* DiffuseLightMaterial material.zig:94-110 (emit texture) */
} rtw_wmaterial_kind;
typedef struct {
  uint32_t kind, tex;
  double albedo[3];
  double fuzz, ir;
} rtw_wmaterial;

typedef struct {              /* Perlin, perlin.zig:10-40 */
  double ranvec[256][3];
  uint32_t perm[3][256];
} rtw_perlin;

typedef struct {              /* decoded texture image: RGBA8, row-major, top row first */
  uint32_t width, height;
  const uint8_t *rgba;
} rtw_image;

typedef struct {
  const rtw_prim *prims;          uint32_t n_prims;
  const rtw_xform *xforms;        uint32_t n_xforms;
  const rtw_texture *textures;    uint32_t n_textures;
  const rtw_wmaterial *mats;      uint32_t n_mats;
  const rtw_perlin *perlins;      uint32_t n_perlins;
  const rtw_image *images;        uint32_t n_images;
} rtw_world_desc;

/* Camera / image settings a scene sets in main() (main.zig:303-376). */
typedef struct {
  double look_from[3], look_at[3], vfov, aperture, aspect;
  double background[3];
  uint32_t width, height, spp, reserved;
} rtw_scene_settings;

/* Scene builders of main.zig on DefaultPrng.init(seed): 1 cover (:157),
 * 2 two spheres (:123), 3 two Perlin spheres (:140), 4 earth (:223),
 * 5 simple light (:235), 6 Cornell box (:256), 7 globe + 10k random spheres
 * (configs[4]; not a reference scene).  `image` is the earth texture
 * (scenes 4, 7; pixels are copied).  The built scene owns its arrays;
 * rtw_built_scene_desc points into them until rtw_built_scene_free. */
typedef struct rtw_built_scene_s *rtw_built_scene;
int rtw_build_scene(uint32_t scene_id, uint64_t seed, const rtw_image *image, rtw_built_scene *out);
int rtw_built_scene_desc(rtw_built_scene b, rtw_world_desc *desc, rtw_scene_settings *settings,
                         uint64_t rng_state_after[4]);
int rtw_built_scene_free(rtw_built_scene b);

/* Upload a world to the CURRENT device: tables + a BVH over worlds of more
 * than 32 primitives (flags bit 0 = RTW_WORLD_LINEAR: no BVH, every segment
 * tests every primitive in a wave-uniform loop; bit 1 = RTW_WORLD_DEBUG_BVH;
 * bit 2 = RTW_WORLD_DYNAMIC, "dynamic worlds" below). */
#define RTW_WORLD_LINEAR 1u
#define RTW_WORLD_DEBUG_BVH 2u /* diagnostic: the BVH root's two children (leaf / node, boxes) to stderr */
typedef struct rtw_world_s *rtw_world;
int rtw_world_create(const rtw_world_desc *desc, uint32_t flags, rtw_world *out);
int rtw_world_destroy(rtw_world world);
/* BVH statistics: nodes, leaves, max depth, max leaf size. */
int rtw_world_bvh_info(rtw_world world, uint32_t info_out[4]);

/* ---- dynamic worlds: new numbers for an uploaded world, in place ----------
 * A world created with RTW_WORLD_DYNAMIC (rtw_world_create flags bit 2) can
 * take new geometry numbers without being created again: each primitive's
 * a[9] and each transform's v[][3].  Everything else is fixed at creation:
 * kinds, materials, transform indices, op lists, textures, counts, and the
 * BVH's topology (its refs, the stored order, rtw_world_bvh_info) — the
 * tree is refitted, not rebuilt.  A DYNAMIC world keeps a small host copy of
 * the fixed fields and a second device allocation (the refit's tables, freed
 * by rtw_world_destroy); a world without the flag allocates nothing extra,
 * its tables are the same bytes, and both entries return RTW_EINVAL for it.
 * A DYNAMIC world without a BVH (<= 32 primitives, or RTW_WORLD_LINEAR)
 * updates its records only.
 *
 * rtw_world_update takes HOST arrays shaped like the descriptor's, checks
 * that their fixed fields equal the world's (else RTW_EINVAL), and runs on
 * the null stream.  rtw_world_update_device takes bare doubles in DEVICE
 * memory of the world's device: d_a is n_prims x 9 in list order, d_xv is
 * n_xforms x RTW_MAX_XFORM_OPS x 3 or NULL (the transforms keep their values);
 * the arrays must stay valid until the work enqueued on `stream` has run.
 *
 * Validate, then commit.  A first phase only reads the input: every number a
 * primitive's kind uses (and every value of a transform's ops) must be finite
 * and a moving sphere needs t1 > t0; the same pass reduces the world's f64
 * box and the leaf pretest's bounds.  The host waits for that one small
 * readback — the call's only synchronisation.  On a violation the call
 * returns RTW_EINVAL with a message and the world is untouched.  Otherwise the
 * commit kernels are enqueued on `stream` and the call returns without
 * waiting: work enqueued later on that stream sees the new world.  An update
 * while a render or query of the same world is in flight on ANOTHER stream is
 * the caller's race.
 *
 * Contract: after an update, every render, guide buffer and ray query of the
 * world is byte-identical to that of a world freshly created from the updated
 * description (any engine choice, traversal, feature set or accumulator
 * state), hence to the oracle.  The device tables themselves are specified
 * too: they equal rtw_world_refit_tables_host of the same numbers byte for
 * byte, and an update with the creation's own numbers reproduces the created
 * tables.
 *
 * Leaf pretest under motion: a leaf keeps its pretest iff it had a record at
 * creation and each of its spheres still qualifies (untransformed, |r| < 100,
 * static or moving over the shutter [0, 1]); when the update's Cmax (the
 * largest |centre| + |centre1 - centre0| over those leaves) exceeds 2^20
 * every leaf loses it until a later update is back within the limit.  A world
 * that had no pretest table at creation never gets one.  All of this changes
 * speed only, never a result.
 *
 * Tree quality degrades as primitives move far from where the builder put
 * them: boxes grow and overlap.  rtw_world_bvh_cost measures that and
 * rtw_world_rebuild* gives the world a new tree in place ("rebuild" below);
 * nothing rebuilds on its own. */
#define RTW_WORLD_DYNAMIC 4u
int rtw_world_update(rtw_world w, const rtw_prim *prims, uint32_t n_prims,
                     const rtw_xform *xforms, uint32_t n_xforms);
int rtw_world_update_device(rtw_world w, const double *d_a, const double *d_xv, void *stream);
/* Diagnostics (tests): the size of the world's device tables; a synchronous
 * copy of them with cull_out = {cull_cmax, cull_rho} and bounds_out = the
 * world box {lo[3], hi[3]} (any world; bytes must equal the size); and what
 * the tables of `desc` created with `flags` hold after an update with a / xv
 * (HOST arrays shaped as rtw_world_update_device's; a == NULL: as created),
 * computed on the host alone.  RTW_EINVAL where the update would refuse. */
size_t rtw_world_table_bytes(rtw_world w);
int rtw_world_read_tables(rtw_world w, void *out, size_t bytes, float cull_out[2], double bounds_out[6]);
int rtw_world_refit_tables_host(const rtw_world_desc *desc, uint32_t flags, const double *a, const double *xv,
                                void *out, size_t bytes, float cull_out[2], double bounds_out[6]);

/* ---- rebuild: a new tree for a dynamic world, on the device ----------------
 * rtw_world_rebuild / rtw_world_rebuild_device take the arguments of
 * rtw_world_update / rtw_world_update_device, run the same checks in the same
 * validate-then-commit order, and also choose a new topology from the new
 * numbers: a rebuild is an update that re-sorts the primitives.  Supported:
 * DYNAMIC worlds whose BVH has leaves of one primitive (rtw_world_bvh_info's
 * largest leaf == 1: worlds of >= 512 primitives).  Such a tree is a full
 * binary tree of n_prims - 1 nodes, so node count, leaf count, largest leaf
 * and every table's size stay; only the depth in rtw_world_bvh_info may
 * change.  Any other world with the flag (no BVH, RTW_WORLD_LINEAR, leaves of
 * two) gets RTW_UNSUPPORTED, a world without it RTW_EINVAL; a refused call
 * leaves the world byte for byte as it was.
 *
 * The tree: each primitive's key is the 63-bit Morton code of its box's f64
 * centroid inside the box of all centroids (21 bits per axis, x highest); the
 * new stored order is the stable sort of the list by key.  Top-down over the
 * sorted range, a node splits where the highest differing key bit changes
 * while a median subtree of the rest still fits the depth cap (the per-lane
 * walk's stack when ceil(log2 n_prims) fits it, so that walk stays
 * available; else the union walk's), and at the median after that or when all
 * its keys are equal.  Records are numbered breadth-first.  Bounds, packed
 * refs, pretest records and the world box are the update's commit run over the
 * new tree; which leaves may hold a pretest record is judged anew on the
 * rebuild's numbers.
 *
 * Contract: after a rebuild every render, guide buffer, ray query and
 * accumulator pass equals that of a world freshly created from the same
 * numbers, byte for byte; later updates refit the new topology.  The tables,
 * cull scalars, bounds and bvh_info equal rtw_world_rebuild_tables_host of the
 * same numbers (info_out: rtw_world_bvh_info's): a function of the numbers,
 * not of the history of updates and rebuilds.
 * rtw_world_rebuild_refit_tables_host: the same, followed by an update with
 * a2 / xv2 (a2 == NULL: none).
 *
 * The first rebuild makes a third device allocation (keys, the sort's storage,
 * the staged topology) that the world keeps.  A rebuild waits once, for the
 * update's readback widened by the new depth and the nodes per level, after
 * validation and before anything is written.
 *
 * rtw_world_bvh_cost: the sum over nodes of (half-area(child 0 box) +
 * half-area(child 1 box)) / half-area(root box), the boxes as the node table
 * stores them, the root box the union of the root's two; summed in f64 in a
 * fixed order, so two calls agree to the bit.  Any world with a BVH, DYNAMIC or
 * not (else RTW_UNSUPPORTED); waits for its 8-byte readback on `stream`.  Its
 * ratio to the cost right after creation or the last rebuild tells when a
 * rebuild pays. */
int rtw_world_rebuild(rtw_world w, const rtw_prim *prims, uint32_t n_prims,
                      const rtw_xform *xforms, uint32_t n_xforms);
int rtw_world_rebuild_device(rtw_world w, const double *d_a, const double *d_xv, void *stream);
int rtw_world_bvh_cost(rtw_world w, void *stream, double *cost_out);
int rtw_world_rebuild_tables_host(const rtw_world_desc *desc, uint32_t flags, const double *a, const double *xv,
                                  void *out, size_t bytes, float cull_out[2], double bounds_out[6], uint32_t info_out[4]);
int rtw_world_rebuild_refit_tables_host(const rtw_world_desc *desc, uint32_t flags, const double *a, const double *xv,
                                        const double *a2, const double *xv2, void *out, size_t bytes,
                                        float cull_out[2], double bounds_out[6], uint32_t info_out[4]);

/* Device workspace of a world render on the CURRENT device (the world's):
 * rtw_workspace_bytes(params) + the tail dealing's per-lane sample rings
 * (one per lane of the persistent grid).  The rings live in the caller's
 * workspace, so renders on different streams, each with its own workspace,
 * are independent.  0 on error. */
size_t rtw_world_workspace_bytes(rtw_world world, const rtw_params *params);
/* Asynchronous render of a world (params.precision must be F64, engine
 * MEGAKERNEL); workspace sized by rtw_world_workspace_bytes(world, params).
 * A workspace of only rtw_workspace_bytes(params) bytes renders without tail
 * dealing (the same image, a few % slower on the large scenes). */
int rtw_world_render_device(rtw_world world, const rtw_camera *cam, const rtw_params *params,
                            void *workspace, size_t workspace_bytes, uint8_t *d_rgb, float *d_mean,
                            void *stream, rtw_timer timer);
/* Synchronous host-buffer render of a world description. */
int rtw_world_render(const rtw_camera *cam, const rtw_world_desc *desc, const rtw_params *params,
                     uint8_t *rgb_out, float *mean_out);
/* How a render of `world` with `params` would launch on the current device
 * (the world's): info_out[6] = {traversal (rtw_world_traversal: LANE, UNION
 * or LINEAR, after AUTO and the world's limits are applied), kernel feature
 * set, register budget (waves per SIMD: 4, 3, or 1 = unconstrained),
 * workgroups per CU, persistent grid (workgroups), dynamic LDS bytes per
 * workgroup}. */
int rtw_world_launch_info(rtw_world world, const rtw_params *params, uint32_t info_out[6]);
/* Statistics pass: counts_out[4] = {samples, segments, node_visits, prim_tests}. */
int rtw_world_render_counts(rtw_world world, const rtw_camera *cam, const rtw_params *params,
                            void *workspace, size_t workspace_bytes, uint64_t counts_out[4]);
/* The same pass with counts_out[8]: the four above (node visits and primitive
 * tests counted per lane: each lane's own under the per-lane traversal, the
 * wave's under the union walk), then the wave iterations of the persistent
 * kernel, whether tail dealing ran (1: the workspace held the per-lane rings,
 * 0: it did not — same image, slower end of launch), and the per-lane
 * traversal's interior-step and leaf-test wave iterations (0 for the union). */
int rtw_world_render_counts_ex(rtw_world world, const rtw_camera *cam, const rtw_params *params,
                               void *workspace, size_t workspace_bytes, uint64_t counts_out[8]);

/* ============================================= progressive rendering ===
 * A frame accumulated over sample passes: render some samples, look at the
 * image, render more, stop on a sample or a noise budget, save the state and
 * resume it.  The accumulator holds the frame's running f64 pixel sum and a
 * per-pixel luminance statistic (rows * W * 40 bytes of device memory); a
 * pass needs the workspace of its own samples only, so device memory no
 * longer grows with the frame's spp.
 *
 * Contract: after passes totalling N samples, the resolved rgb8 and mean are
 * byte-identical to a one-shot render (rtw_render_device /
 * rtw_world_render_device) of the same params with spp = N, whenever N is a
 * multiple of the chunk or equals params->spp — for every engine, precision,
 * row shard and world.  The chunk is the one-shot's:
 * min(params->chunk ? params->chunk : RTW_DEFAULT_CHUNK, params->spp).
 *
 * Pass rules: pass_spp >= 1; done + pass_spp <= params->spp; pass_spp is a
 * multiple of the chunk unless the pass is the frame's last
 * (done + pass_spp == params->spp).  A violation returns RTW_EINVAL, sets the
 * message and leaves the accumulator untouched.
 *
 * Calling conventions: the passes, resolves and noise queries of one
 * accumulator are issued on one stream, on the accumulator's device.  The
 * count of samples done is HOST state, advanced when a pass is enqueued, and
 * a pass's sample range is fixed at that moment: a captured graph of a pass
 * would replay the SAME samples, so passes are not to be replayed from a
 * graph.  The wavefront engine's passes cannot be captured at all
 * (rtw_render_device). */
typedef struct rtw_accum_s *rtw_accum;

/* An empty accumulator (sums zeroed) on the CURRENT device.  params is copied:
 * every pass renders with its size, rows, seed, depth, background, precision,
 * engine and engine knobs; params->spp is the frame's total. */
int rtw_accum_create(const rtw_params *params, rtw_accum *out);
int rtw_accum_destroy(rtw_accum a);
/* Samples accumulated so far (enqueued passes included). */
int rtw_accum_samples(rtw_accum a, uint32_t *done);

/* Device workspace of a pass of pass_spp samples: rtw_workspace_bytes /
 * rtw_world_workspace_bytes of params with spp = pass_spp.  0 unless pass_spp
 * is a multiple of the chunk or equals params->spp.  (A shorter last pass fits
 * the workspace of the next multiple of the chunk.) */
size_t rtw_accum_workspace_bytes(const rtw_params *params, uint32_t pass_spp);
size_t rtw_accum_world_workspace_bytes(rtw_world w, const rtw_params *params, uint32_t pass_spp);

/* One pass: samples [done, done + pass_spp) of every pixel, asynchronous on
 * `stream` — the render of rtw_render_device / rtw_world_render_device with
 * spp = pass_spp, started `done` samples into each pixel's random stream,
 * its chunk sums folded into the accumulator where the one-shot render
 * launches its finalize kernel.  timer (optional) brackets the trace kernel(s).
 * A world pass in a workspace of only rtw_accum_workspace_bytes runs without
 * tail dealing (the same sums). */
int rtw_accum_render_device(rtw_accum a, rtw_scene scene, const rtw_camera *cam, uint32_t pass_spp,
                            void *workspace, size_t workspace_bytes, void *stream, rtw_timer timer);
int rtw_accum_world_render_device(rtw_accum a, rtw_world world, const rtw_camera *cam, uint32_t pass_spp,
                                  void *workspace, size_t workspace_bytes, void *stream, rtw_timer timer);

/* The image of the samples done so far, asynchronous on `stream`: d_rgb
 * (W*row_count*3 bytes) and optional d_mean (W*row_count*3 floats) =
 * sum / done, quantised as the one-shot render does.  RTW_EINVAL before the
 * first pass. */
int rtw_accum_resolve_device(rtw_accum a, uint8_t *d_rgb, float *d_mean, void *stream);

/* The frame's noise, synchronous: the RMS over the pixels of the standard
 * error of the pixel's mean luminance, sqrt(sum_pix se2 / npix) with
 * se2 = max(0, SY2 - SY*SY/m) / (m*(m-1)*n_c*n_c), where SY and SY2 sum Y and
 * Y*Y over the m full chunks accumulated, Y = (0.2126 r + 0.7152 g) + 0.0722 b
 * of a chunk's sum and n_c is the chunk.  Deterministic: the same state gives
 * the same bits.  RTW_EINVAL with fewer than 2 full chunks. */
int rtw_accum_noise(rtw_accum a, void *stream, double *noise);

/* Save and resume, HOST buffers, synchronous (they wait for the device):
 * sum (npix*3) is the running pixel sum, stat (npix*2; optional in _read) the
 * luminance statistic {SY, SY2}, npix = W*row_count.  rtw_accum_load replaces
 * the state; samples_done must be a multiple of the chunk or params->spp. */
int rtw_accum_read(rtw_accum a, double *sum_out, double *stat_out);
int rtw_accum_load(rtw_accum a, const double *sum, const double *stat, uint32_t samples_done);

/* ---- adaptive sampling: masked passes and a per-pixel noise budget ----
 *   The first rtw_accum_set_mask, rtw_accum_set_adaptive
 * (tol > 0) or rtw_accum_load_counts puts the accumulator in the MASKED state,
 * for good: it then keeps a per-pixel sample count and an active set.
 *
 * A pixel is active while it has received every sample so far (count ==
 * samples done), the mask keeps it and the budget has not found it converged.
 * Once inactive it stays inactive: a later pass covers samples
 * [done, done + pass_spp) for all pixels alike, so a pixel that skipped a pass
 * could no longer hold a prefix of its sample stream.  A pass renders the
 * active pixels only (the launch covers only the 8x8 tiles that hold one) and
 * the fold touches nothing of an inactive pixel.
 *
 * Contract, per pixel: a pixel whose count is n holds the bytes of the
 * one-shot render with spp = n at that pixel — rgb8, mean, and the running
 * sum — for every engine, precision, row shard and world, whenever n is a
 * multiple of the chunk or params->spp.  rtw_accum_resolve_device divides
 * each pixel by its own count (a pixel with no sample resolves to 0).
 *
 * Synchronisation: in the masked state rtw_accum_render_device /
 * rtw_accum_world_render_device first WAIT, on the host, for the active-set
 * update of the previous pass and read back its active-tile count (one 8-byte
 * copy per pass) to size the launch; the pass itself is asynchronous as
 * before.  With no active pixel they launch nothing, change nothing and
 * return RTW_OK; rtw_accum_samples advances only when something was launched,
 * and a timer passed to such a pass holds no interval (rtw_timer_elapsed_ms
 * returns RTW_EINVAL until it brackets a launch again).
 * A masked pass saves time, not memory: chunk sums go to the pixel's own
 * position, so it needs the same workspace as an unmasked pass of its
 * pass_spp.  Masked passes, like all passes, are not for graph replay.  A
 * never-masked accumulator pays for none of this and keeps its bytes.
 *
 * Budget: after every fold (and when the budget is set or a state loaded)
 * each active pixel with cnt samples, m = cnt / chunk full chunks and
 * statistic {SY, SY2} is tested, in f64 with one IEEE operation per operator:
 *   se2 = fmax(0, SY2 - SY*SY/m) / (m * (m-1) * n_c * n_c)
 *   converged = m >= 2 && cnt >= min_spp && se2 <= tol*tol
 * — rtw_accum_noise's per-pixel term against an absolute target on the
 * standard error of the pixel's mean luminance.  The test runs once per fold,
 * whatever the pass size. */

/* active &= (mask != 0).  mask: HOST, W*row_count bytes.  Synchronous. */
int rtw_accum_set_mask(rtw_accum a, const uint8_t *mask);
/* tol > 0 sets the budget, 0 removes it (pixels already inactive stay so);
 * applied at once if samples are accumulated.  RTW_EINVAL for a negative or
 * non-finite tol.  Synchronous. */
int rtw_accum_set_adaptive(rtw_accum a, double tol, uint32_t min_spp);
/* Active pixels and the tiles that hold them.  Synchronous. */
int rtw_accum_active(rtw_accum a, uint32_t *pixels, uint32_t *tiles);
/* Per-pixel sample counts, HOST, W*row_count words.  Synchronous. */
int rtw_accum_read_counts(rtw_accum a, uint32_t *cnt_out);
/* rtw_accum_load with per-pixel counts: every cnt <= samples_done, and a
 * multiple of the chunk or params->spp, else RTW_EINVAL and the state is
 * untouched.  Afterwards active = (cnt == samples_done), then the budget if
 * one is set.  A mask is not part of the saved state.  (rtw_accum_load itself:
 * all counts = samples_done, all pixels active, then the budget.)
 * rtw_accum_noise on a masked accumulator uses each pixel's own m, leaves
 * pixels with m < 2 out of the sum and the divisor, and returns RTW_EINVAL if
 * none remains. */
int rtw_accum_load_counts(rtw_accum a, const double *sum, const double *stat, const uint32_t *cnt,
                          uint32_t samples_done);

/* ================================================= feature-guided denoiser ===
 *   An image-space filter for previews and finished frames:
 * first-hit feature buffers ("guides") from a deterministic ray per pixel, and
 * an edge-avoiding a-trous wavelet filter steered by them and by the
 * accumulator's per-pixel luminance variance.  New symbols only: a render
 * without these calls is untouched.
 *
 * Guides.  One record per output pixel, rows in output order like d_rgb.  The
 * feature ray of pixel (x, image row y, top first) draws nothing from the RNG:
 * Camera.getRay (main.zig:91-100) with its two random draws replaced by their
 * means — s = (x + 0.5) / (W - 1), t = ((H - 1 - y) + 0.5) / (H - 1), lens
 * offset 0 (origin = cam.origin, direction = llc + s*horizontal + t*vertical -
 * origin), time = time0 + 0.5 * (time1 - time0), t_min = 0.001, t_max = inf —
 * in f64, each field rounded to f32 on store. */
typedef struct {
  float normal[3];   /* the hit record's normal (facing the ray); 0,0,0 on a miss */
  float depth;       /* ray parameter t of the hit (direction not normalised); 0 on a miss */
  float albedo[3];   /* Lambert: the texture's value at the hit; Metal: its albedo; Dielectric: 1,1,1;
                        Light: the emit texture's value; the frame's background on a miss */
  uint32_t prim;     /* primitive (world) or sphere (scene) list index + 1; 0 on a miss */
} rtw_guide;         /* 32 bytes; buffers of it are 16-byte aligned */

/* Asynchronous on `stream`; d_guides: W * row_count records of device memory.
 * Of params only width, height, row_begin, row_stride, row_count and
 * background matter.  No workspace. */
int rtw_scene_guides_device(rtw_scene scene, const rtw_camera *cam, const rtw_params *params,
                            rtw_guide *d_guides, void *stream);
int rtw_world_guides_device(rtw_world world, const rtw_camera *cam, const rtw_params *params,
                            rtw_guide *d_guides, void *stream);

/* The filter (csrc/rtw_denoise.hpp has the weight functions): `levels`
 * iterations of 5x5 B3-spline taps spaced 1, 2, 4, ... pixels; a tap's weight
 * is the product of the spline weight and of colour, normal, depth and albedo
 * terms; variance is filtered along with the colour.  Every field 0 = its
 * default (5 levels; sigmas 2, 0.1, 0.25, 0.1). */
#define RTW_DENOISE_NO_COLOR 1u   /* flags bit 0: drop the colour term */
#define RTW_DENOISE_DIRECT 2u     /* flags bit 1: every level reads its taps from global memory, none through
                                     LDS tiles (the same bytes; for measurement) */
#define RTW_DENOISE_SPATIAL_VAR 4u /* flags bit 2: before the first level every RTW_VAR_UNKNOWN variance (all of
                                     them when d_var is NULL) is replaced by the spatial estimate below */
#define RTW_DENOISE_MAX_LEVELS 6u
typedef struct {
  uint32_t levels;                /* 1..6, 0 = 5 */
  double sigma_color;             /* in standard errors of the centre's luminance */
  double sigma_normal;            /* 1 - dot(n_p, n_q) at which the normal term reaches 0 */
  double sigma_depth;             /* relative to the larger of the two depths */
  double sigma_albedo;            /* in units of linear albedo */
  uint32_t flags;                 /* RTW_DENOISE_* */
} rtw_denoise_opts;

/* Variance values: >= 0 known; RTW_VAR_UNKNOWN: the colour term is dropped at
 * that pixel; RTW_VAR_EMPTY: the pixel holds no sample — it contributes to
 * nobody and stays 0. */
#define RTW_VAR_UNKNOWN (-1.0f)
#define RTW_VAR_EMPTY (-2.0f)

/* Two ping-pong images of {r, g, b, var} f32.  0 on bad arguments. */
size_t rtw_denoise_workspace_bytes(uint32_t width, uint32_t height, const rtw_denoise_opts *opts);
/* Denoise a W x H image of contiguous rows.  d_mean: W*H*3 floats (linear);
 * d_var: W*H floats (the variance of the pixel's luminance, see above) or NULL
 * (all unknown); d_guides: W*H records or NULL (the guide terms are dropped);
 * opts: NULL = defaults.  Outputs: d_rgb_out (W*H*3 bytes, quantised as a
 * render's) and/or d_mean_out (W*H*3 floats), at least one.  The inputs are
 * not modified and may not alias the outputs.  Plain device buffers,
 * asynchronous on `stream`, graph-capturable; no state, no atomics: the same
 * inputs give the same bytes, and those are rtw_denoise_host's. */
int rtw_denoise_device(const float *d_mean, const float *d_var, const rtw_guide *d_guides, uint32_t width,
                       uint32_t height, const rtw_denoise_opts *opts, void *workspace, size_t workspace_bytes,
                       uint8_t *d_rgb_out, float *d_mean_out, void *stream);
/* The same filter on HOST buffers (workspace included), on the CPU: needs no
 * GPU.  `stream` is ignored. */
int rtw_denoise_host(const float *mean, const float *var, const rtw_guide *guides, uint32_t width,
                     uint32_t height, const rtw_denoise_opts *opts, void *workspace, size_t workspace_bytes,
                     uint8_t *rgb_out, float *mean_out, void *stream);

/* The spatial variance estimate (csrc/rtw_denoise.hpp
 * spatial_variance_pixel): for an image of fewer than two chunks, whose
 * variance the accumulator does not know yet.  var_out (W*H floats) = var_in
 * with every RTW_VAR_UNKNOWN pixel replaced by the guide-weighted variance of
 * the mean's luminance over the pixel's 7x7 window — weights: the filter's
 * normal, depth and albedo terms with the call's sigmas, 1 without guides;
 * taps outside the image, empty taps and taps across the hit / miss border
 * dropped.  Known (>= 0) and RTW_VAR_EMPTY pixels come back bit for bit; a
 * pixel with fewer than 4 usable taps stays RTW_VAR_UNKNOWN.  var_in NULL:
 * all unknown; guides NULL: unweighted.  Of opts only the three guide sigmas
 * and RTW_DENOISE_DIRECT (the device reads its taps from global memory, not
 * through an LDS tile: the same bytes) matter.  No workspace; var_out may not
 * alias an input.  The device form is asynchronous on `stream`,
 * graph-capturable, without atomics, and gives the host form's bytes.
 * rtw_denoise_* with RTW_DENOISE_SPATIAL_VAR give the bytes of the unflagged
 * call on this map; the workspace sizes are the unflagged ones. */
int rtw_denoise_spatial_variance_device(const float *d_mean, const float *d_var_in, const rtw_guide *d_guides,
                                        uint32_t width, uint32_t height, const rtw_denoise_opts *opts,
                                        float *d_var_out, void *stream);
int rtw_denoise_spatial_variance_host(const float *mean, const float *var_in, const rtw_guide *guides,
                                      uint32_t width, uint32_t height, const rtw_denoise_opts *opts, float *var_out,
                                      void *stream);

/* The accumulator's per-pixel variance, asynchronous on `stream`: d_var
 * (W*row_count floats) = f32 of the squared standard error of the pixel's mean
 * luminance (rtw_accum_noise's per-pixel term, in the mean image's units),
 * each pixel with its own m = count / chunk in the masked state;
 * RTW_VAR_UNKNOWN where m < 2, RTW_VAR_EMPTY where the pixel has no sample. */
int rtw_accum_variance_device(rtw_accum a, float *d_var, void *stream);
/* Resolve, variance, filter: the denoised image of the samples so far into
 * d_rgb and/or d_mean (optional each, not both NULL).  d_guides may be NULL.
 * workspace: rtw_accum_denoise_workspace_bytes(a, opts) bytes of device memory,
 * 16-byte aligned — the filter's two images plus the resolved mean, the
 * variance and the resolve's rgb8 (19 bytes per pixel).  The accumulator's
 * state is not modified: passes may continue.  Rows must be contiguous image
 * rows: RTW_UNSUPPORTED when params.row_stride != 1.  With
 * RTW_DENOISE_SPATIAL_VAR the pixels with m < 2 — every pixel after a single
 * chunk — get the spatial estimate; RTW_VAR_EMPTY pixels stay empty and 0. */
size_t rtw_accum_denoise_workspace_bytes(rtw_accum a, const rtw_denoise_opts *opts);
int rtw_accum_denoise_device(rtw_accum a, const rtw_guide *d_guides, const rtw_denoise_opts *opts,
                             void *workspace, size_t workspace_bytes, uint8_t *d_rgb, float *d_mean,
                             void *stream);

/* ============================================================ ray queries ===
 *   The closest hit, or the occlusion, of rays the CALLER
 * supplies, over an uploaded world or scene: picking the primitive under a
 * pixel, visibility and shadow tests, ambient occlusion, an integrator of the
 * caller's own.  New symbols only: a render without these calls is untouched.
 *
 * Closest hit.  The answer is HittableList.hit's (hittable.zig:231-244) over
 * the flattened list: the minimal accepted root in [t_min, t_max]; a root equal
 * to the current closest is accepted, so among equal roots the later list index
 * wins.
 * Hit record.  The reference's HitRecord: p, and the normal facing the ray;
 * front = 1 if the outward normal opposes the ray; u, v = getSphereUv for a
 * static sphere, 0, 0 for a moving sphere, (x - a0) / (a1 - a0),
 * (y - b0) / (b1 - b0) for a rect; Translate / RotateY wrappers applied back in
 * the reference's order; prim = list index + 1 as in rtw_guide (the sphere
 * index + 1 for a scene).  A miss: all 80 bytes 0.
 * Occlusion.  d_occluded[i] = 1 iff the closest-hit query of ray i would hit,
 * else 0; the kernel stops a ray at its first accepted root (the answer does
 * not depend on the order).
 * Arithmetic.  f64, one IEEE operation per reference operation, as everywhere
 * in this library; every field of a record equals the oracle's rw_hit
 * (oracle/rtw_world.h) bit for bit.
 * Input domain.  Components finite, dir != 0, time finite, t_min <= t_max,
 * t_max may be +inf; direction components that are exactly 0 are in the
 * domain, and a NaN root sends the ray through the reference's sequential loop
 * as in a render, over a world and over a scene alike.  Finite components can
 * produce one: where |dir|^2, (origin - centre) . dir or |origin - centre|^2
 * overflows (a direction longer than 2^512) the discriminant is inf - inf,
 * which the reference does not reject; it then accepts every later sphere
 * whose discriminant is not negative, so the record is the last such sphere of
 * the list with t = NaN (p, normal, u, v follow from that t) and the ray is
 * occluded.  A direction so short that |dir|^2 underflows to 0 has roots of
 * +-inf; +inf is accepted like any root.  (A ray whose time lies outside [0, 1]
 * on a world whose BVH holds moving spheres takes the sequential loop too: the
 * boxes cover those times only.  A scene extrapolates a moving sphere's centre
 * linearly outside its own [t0, t1], as the reference does.)
 * The BVH's box tests (not the primitive tests) give a direction component that
 * is 0, or smaller than 2^-60 of the largest, that magnitude: the slab
 * arithmetic divides by it, and the shift stays far inside the boxes' margin.
 * A ray that lies in a rect's plane (the reference's 0/0, whose answer depends
 * on the list order) is guaranteed the reference's record only in worlds
 * without a BVH: a walk meets that rect only where the ray meets its box.
 * Outside the domain the record's contents are unspecified, but no access
 * leaves the tables or the output buffers: the stack depth bounds every walk.
 * Launch.  The _device entries are asynchronous on `stream`: one kernel launch,
 * no allocation, no synchronisation, no atomics on the outputs; the same input
 * gives the same bytes.  n == 0 returns RTW_OK and launches nothing.
 * RTW_EINVAL for null pointers, d_rays / d_hits not 8-byte aligned, or
 * n > 2^31.  The world or scene must live on the current device.  Capture into
 * a graph is not tested and not promised.
 * Traversal (opts->traversal, opts NULL = all 0): UNION and LANE are forced as
 * in rtw_params.world_traversal; a world that cannot walk per lane (not a
 * sphere world, or no BVH) takes the union walk or the linear loop —
 * rtw_world_query_info says which.  AUTO: see RTW_QUERY_LANE_NODES. */
typedef struct { double origin[3], dir[3]; double time, t_min, t_max; } rtw_ray;            /* 72 bytes */
typedef struct { double t, p[3], normal[3], u, v; uint32_t prim, front; } rtw_hit;          /* 80 bytes */
typedef struct {
  uint32_t traversal;  /* rtw_world_traversal, 0 = AUTO */
  uint32_t flags;      /* 0 */
} rtw_query_opts;
#define RTW_QUERY_MAX_RAYS (1ull << 31)
/* AUTO: per lane for sphere worlds whose BVH has at least this many nodes, else
 * the union walk — rtw_params.world_traversal's rule, which the measurement on
 * incoherent rays (one bounce per hit of a frame's feature rays; tools/
 * query_bench.py, profiles/r13/query.txt) confirms at both ends: the globe
 * (9,981 nodes) 0.1723 ms per lane against 0.1930 ms union for 651,951 rays,
 * scene 1 (23 nodes) 0.0452 ms union against 0.0645 ms per lane for 810,089. */
#define RTW_QUERY_LANE_NODES 256u

/* Host helper: the feature ray of pixel (x, image row y, top first) exactly as
 * the guides define it ("Guides" above: s, t at the pixel centre, lens offset
 * 0, mid-shutter time), t_min = 0.001, t_max = +inf.  RTW_EINVAL for null
 * pointers, width or height < 2, x >= width or y >= height. */
int rtw_pixel_ray(const rtw_camera *cam, uint32_t width, uint32_t height, uint32_t x, uint32_t y, rtw_ray *out);

int rtw_world_trace_device(rtw_world w, const rtw_ray *d_rays, uint64_t n, const rtw_query_opts *opts,
                           rtw_hit *d_hits, void *stream);
int rtw_world_occluded_device(rtw_world w, const rtw_ray *d_rays, uint64_t n, const rtw_query_opts *opts,
                              uint8_t *d_occluded, void *stream);
int rtw_scene_trace_device(rtw_scene s, const rtw_ray *d_rays, uint64_t n, rtw_hit *d_hits, void *stream);
int rtw_scene_occluded_device(rtw_scene s, const rtw_ray *d_rays, uint64_t n, uint8_t *d_occluded, void *stream);
/* HOST buffers, synchronous (allocate, copy, trace, copy back): for one-off
 * queries such as a pick. */
int rtw_world_trace(rtw_world w, const rtw_ray *rays, uint64_t n, const rtw_query_opts *opts, rtw_hit *hits_out);
int rtw_scene_trace(rtw_scene s, const rtw_ray *rays, uint64_t n, rtw_hit *hits_out);
/* How a query would launch on this world (current device = the world's) at its
 * largest: info_out[4] = {traversal after AUTO and the world's limits (LANE,
 * UNION or LINEAR), kernel feature set, workgroups of a batch that fills the
 * device (a smaller batch launches ceil(n / 256)), dynamic LDS bytes per
 * workgroup}. */
int rtw_world_query_info(rtw_world w, const rtw_query_opts *opts, uint32_t info_out[4]);
/* Host reference of the triangle primitive (no device involved): the closest hit
 * of each ray over the description's TRIANGLE primitives only — every other
 * kind is skipped — by the reference's sequential list loop, chains included,
 * through the arithmetic the kernels run (csrc/rtw_tri.hpp).  Records as
 * rtw_world_trace's (prim = list index + 1, a miss all zero).  For tests and
 * for integrators that want a CPU twin; merged with the oracle's record of the
 * other kinds (the smaller t, the later list index on a tie) it is the record
 * rtw_world_trace_device returns.  RTW_EINVAL for null pointers, or a triangle
 * with a chain out of range, a non-finite vertex or zero area. */
int rtw_world_trace_tri_host(const rtw_world_desc *desc, const rtw_ray *rays, size_t n, const rtw_query_opts *opts,
                             rtw_hit *hits_out);

/* ======================================================== surface queries ===
 *   What the surface under a hit record IS: its material's
 * kind and index, the value of its texture at the record's u, v, p — a checker,
 * Perlin noise or an image evaluated by the render's own functions — what a
 * light emits there, a metal's fuzz, a glass's index; and, from the same
 * numbers, the rtw_guide record of that ray.  The hit records are those of
 * rtw_world_trace_device / rtw_scene_trace_device over the SAME world or scene
 * in its current state.  New symbols only: nothing else changes.
 *
 * Per record.  prim == 0, or prim beyond the list (the kernel checks this
 * itself: the records are the caller's memory), is a miss: the surface record
 * is 64 zero bytes, the guide {0,0,0, 0, f32(background), 0}.  Otherwise the
 * material is that of list entry prim - 1, and the guide is {f32(normal),
 * f32(t), f32(value), prim}, each f64 rounded to f32 once.
 * Equalities.  For the hits of a frame's feature rays (rtw_pixel_rays_device,
 * then a trace) d_guides equals the buffer of rtw_world_guides_device /
 * rtw_scene_guides_device of that frame byte for byte; every f64 field equals
 * the oracle's (oracle/rtw_world.h rw_texture_value on rw_hit's uv and p, and
 * the material table).
 * Scenes.  The cover scene's table is reported in the world's enumerations:
 * RTW_LAMBERT_SOLID is RTW_WMAT_LAMBERT over RTW_TEX_SOLID, RTW_LAMBERT_CHECKER
 * the same over RTW_TEX_CHECKER; `mat` indexes the scene's material array and
 * tex is 0, a scene having no texture table.
 * Launch.  One kernel launch, asynchronous on `stream`; no allocation, no
 * workspace, no synchronisation, no atomics: the same input gives the same
 * bytes.  d_surf and d_guides are optional each, at least one is required;
 * background may be NULL only when d_guides is.  n == 0 returns RTW_OK and
 * launches nothing.  RTW_EINVAL for a null handle or null d_hits, both outputs
 * NULL, d_guides without background or with a non-finite one, d_hits or d_surf
 * not 8-byte aligned, d_guides not 16-byte aligned, n > 2^31, an output whose n
 * records overlap d_hits' or the other output's anywhere, a world or scene of
 * another device than the current one.
 * Records no trace produced.  The contents of their outputs are unspecified, but
 * no access leaves the tables or the output buffers: prim is bounded as above,
 * every index the tables hold was checked when they were packed, and what u, v
 * and p select — the image's texel, the Perlin lattice point — is clamped or
 * masked before use.  NaN and infinite u, v, p included. */
typedef struct {
  double value[3];   /* Lambert: its texture's value at the record's u, v, p; Metal: its albedo;
                        Dielectric: 1,1,1; Light: its emit texture's value — rtw_guide.albedo before rounding */
  double fuzz;       /* Metal: the number the render's scatter reads; else 0 */
  double ir;         /* Dielectric: likewise; else 0 */
  uint32_t kind;     /* rtw_wmaterial_kind + 1; 0 = a miss */
  uint32_t mat;      /* material index + 1; 0 = a miss */
  uint32_t tex;      /* index + 1 of the texture that gave `value`; 0 = none (Metal, Dielectric, a miss, a scene) */
  uint32_t tex_kind; /* rtw_texture_kind + 1 of that texture; 0 = none */
  uint32_t reserved[2]; /* 0 */
} rtw_surface;       /* 64 bytes, 8-byte aligned */

int rtw_world_surface_device(rtw_world w, const rtw_hit *d_hits, uint64_t n, const double background[3],
                             rtw_surface *d_surf, rtw_guide *d_guides, void *stream);
int rtw_scene_surface_device(rtw_scene s, const rtw_hit *d_hits, uint64_t n, const double background[3],
                             rtw_surface *d_surf, rtw_guide *d_guides, void *stream);
/* HOST buffers, synchronous (allocate, copy, query, copy back): for a pick. */
int rtw_world_surface(rtw_world w, const rtw_hit *hits, uint64_t n, rtw_surface *surf_out);

/* =================================================== temporal accumulation ===
 *   An animation's frames share what they see: each pixel's
 * first-hit surface point is followed back into the previous frame, and where it
 * was visible there the frame's mean is blended into a running mean kept per
 * pixel, with the luminance moments that give the denoiser a variance.  New
 * symbols only: a render without these calls is untouched.  First-hit
 * reprojection only: what a mirror or a glass shows is accumulated at the
 * mirror's own surface point.
 *
 * One frame: render (seed + k: equal seeds give equal noise, which no mean
 * reduces), rtw_pixel_rays_device, rtw_world_trace_device, the guides (off those
 * hits with rtw_world_surface_device, or rtw_world_guides_device: the same bytes),
 * rtw_world_prev_points_device with the previous frame's numbers,
 * rtw_temporal_device, then rtw_denoise_device on d_mean_out with d_var_out as
 * its d_var.  The caller ping-pongs two history images.
 *
 * History record, one per pixel, rows contiguous as for rtw_denoise_device. */
typedef struct {
  float mean[3];   /* accumulated linear colour */
  float len;       /* frames in it; 0: no history */
  float m1, m2;    /* accumulated luminance and squared luminance */
  float depth;     /* the guide's depth and prim of the frame that wrote the record: */
  uint32_t prim;   /* the next frame checks visibility against them */
} rtw_history;     /* 32 bytes; buffers of it are 16-byte aligned */

typedef struct {   /* every field 0 = its default */
  uint32_t max_history;  /* 1..4096, default 32: the blend weight never falls below 1 / (max_history + 1) */
  double depth_tol;      /* finite, > 0, default 0.02: relative to the larger of the two depths */
  uint32_t min_len_var;  /* >= 2, default 4: shorter histories report RTW_VAR_UNKNOWN */
  uint32_t flags;        /* 0 */
} rtw_temporal_opts;

/* Per pixel (x, image row y) — csrc/rtw_temporal.hpp has the arithmetic, f64 with
 * one IEEE operation per operator, each output rounded to f32 once; the device's
 * bytes are the host's:
 *  1. Where it was.  A hit pixel (guide prim != 0) with d_prev_p: the point is
 *     projected through cam_prev (Cramer's rule on d0 + s h + t v = mu q, q = the
 *     point - origin, d0 = lower_left_corner - origin); invalid when an input is
 *     not finite, the determinant is 0 or mu <= 0; fx = s (W - 1) - 0.5,
 *     fy = (H - 1) + 0.5 - t (H - 1), expected depth tp = 1 / mu; an fx or fy
 *     within 2^-10 of an integer becomes that integer.  A hit pixel with
 *     d_prev_p == NULL (nothing moved): its own position, tp = its depth.  A miss:
 *     its own position if cam_prev and cam are bytewise equal, else no history.
 *  2. The four bilinear taps around (fx, fy): a tap counts iff it lies inside the
 *     image, its record has len > 0 and the pixel's prim, and for a hit
 *     |rec.depth - tp| <= depth_tol * max(rec.depth, tp).  Their weights summed in
 *     row-major order below 2^-7: no history.
 *  3. No history: {mean, len 1, m1 = Y, m2 = Y Y}.  Else hist = the
 *     weight-normalised taps, N = min(hist.len, max_history), a = 1 / (N + 1),
 *     colour, m1, m2 = hist + a (cur - hist), len = N + 1.  depth, prim: the guide's.
 *  4. d_var_out = max(0, m2 - m1 m1) / len when len >= min_len_var, else
 *     RTW_VAR_UNKNOWN.
 * d_hist_in == NULL: the first frame, no pixel has history.  d_mean_out
 * (W*H*3 floats, the record's mean) and d_var_out (W*H floats) are optional,
 * d_hist_out is required; outputs may not alias inputs.  d_prev_p: W*H*3 doubles
 * or NULL.  Asynchronous on `stream`, graph-capturable, no workspace, no state, no
 * atomics: the same inputs give the same bytes.  RTW_EINVAL for null pointers,
 * width or height < 2 or > 65536, more than 2^28 pixels (an 8-GiB history image),
 * history or guides not 16-byte aligned, d_prev_p not 8-byte aligned, a float
 * image not 4-byte aligned, an output whose W*H records overlap an input's or
 * another output's anywhere (byte ranges are compared, not only the pointers),
 * opts out of range (opts NULL = defaults). */
int rtw_temporal_device(const float *d_mean, const rtw_guide *d_guides, const double *d_prev_p,
                        const rtw_camera *cam_prev, const rtw_camera *cam,
                        const rtw_history *d_hist_in, uint32_t width, uint32_t height,
                        const rtw_temporal_opts *opts, rtw_history *d_hist_out,
                        float *d_mean_out, float *d_var_out, void *stream);
/* The same on HOST buffers, on the CPU: needs no GPU.  `stream` is ignored. */
int rtw_temporal_host(const float *mean, const rtw_guide *guides, const double *prev_p,
                      const rtw_camera *cam_prev, const rtw_camera *cam,
                      const rtw_history *hist_in, uint32_t width, uint32_t height,
                      const rtw_temporal_opts *opts, rtw_history *hist_out,
                      float *mean_out, float *var_out, void *stream);

/* The same accumulation with the history clamped to the current frame's
 * neighbourhood: what a mirror or a glass shows moves although
 * its surface point does not, and a history that no longer resembles the frame
 * around the pixel is pulled into that frame's range before the blend.  New
 * symbols only; rtw_temporal_device and rtw_temporal_host are untouched. */
typedef struct {     /* every field 0 = its default */
  double gamma;      /* finite, >= 0, < 1e30; 0 = the default, 0.5: the window's mean +- gamma sigma */
  uint32_t radius;   /* 0 = default 1; 1..3: a (2r+1)^2 window */
  uint32_t reserved; /* 0 */
} rtw_temporal_clamp; /* 16 bytes */

/* Steps 1 and 2 above unchanged.  Where the pixel has history, between "hist =
 * the weight-normalised taps" and the blend (csrc/rtw_temporal_clamp.hpp; the
 * same arithmetic rules, and sqrt):
 *  a. Over the pixels (x + dx, y + dy), |dx|, |dy| <= radius, of d_mean in
 *     row-major order, leaving out those outside the image and those with a
 *     non-finite channel, n pixels: per channel mu = s / n, var = max(0, s2 / n -
 *     mu mu), lo = mu - gamma sqrt(var), hi = mu + gamma sqrt(var).
 *  b. n < 4: the history is left alone.  Else each channel of hist becomes
 *     min(max(h, lo), hi).
 *  c. If no channel changed nothing else does: the bytes are rtw_temporal_device's.
 *     Else with d = luminance(h') - luminance(h): m2 = (m2 + (2 m1) d) + d d, then
 *     m1 = m1 + d (the accumulated luminances move with the mean and keep their
 *     variance); len is untouched.
 * Steps 3 and 4 run on the result; a value that comes out NaN (a bad pixel in the
 * frame or in the history) is stored as the quiet NaN 0x7FC00000, whatever NaN
 * the instruction set produced.  clamp == NULL: exactly rtw_temporal_device /
 * rtw_temporal_host.  Every argument check of rtw_temporal_device applies, and
 * RTW_EINVAL also for a non-finite or negative gamma, gamma >= 1e30, radius > 3 or
 * reserved != 0.  Asynchronous on `stream`, graph-capturable, no workspace, no
 * state, no atomics; the device's bytes are the host's. */
int rtw_temporal_clamped_device(const float *d_mean, const rtw_guide *d_guides, const double *d_prev_p,
                                const rtw_camera *cam_prev, const rtw_camera *cam,
                                const rtw_history *d_hist_in, uint32_t width, uint32_t height,
                                const rtw_temporal_opts *opts, const rtw_temporal_clamp *clamp,
                                rtw_history *d_hist_out, float *d_mean_out, float *d_var_out, void *stream);
int rtw_temporal_clamped_host(const float *mean, const rtw_guide *guides, const double *prev_p,
                              const rtw_camera *cam_prev, const rtw_camera *cam,
                              const rtw_history *hist_in, uint32_t width, uint32_t height,
                              const rtw_temporal_opts *opts, const rtw_temporal_clamp *clamp,
                              rtw_history *hist_out, float *mean_out, float *var_out, void *stream);

/* The width*height feature rays of a frame in row-major order, each record
 * byte-equal to rtw_pixel_ray's.  Asynchronous on `stream`.  RTW_EINVAL for null
 * pointers, width or height < 2, more than 2^31 pixels, d_rays not 8-byte aligned. */
int rtw_pixel_rays_device(const rtw_camera *cam, uint32_t width, uint32_t height, rtw_ray *d_rays, void *stream);

/* For each hit record of the world as it is NOW, the same surface point under the
 * PREVIOUS frame's numbers: d_a_prev (n_prims x 9) and d_xv_prev (n_xforms x
 * RTW_MAX_XFORM_OPS x 3) shaped as rtw_world_update_device's, NULL = this frame's
 * values.  Any uploaded world.  d_prev_p: n x 3 doubles.  The surface
 * parametrisation comes from the record alone, nothing is inverted numerically:
 * a sphere's outward object-space normal is the record's normal (negated when
 * front == 0) taken back through the primitive's current transform chain as a
 * direction, and the point is c_prev + r_prev * n (a moving sphere's centre at
 * `time`, c0 + (c1 - c0) * ((time - t0) / (t1 - t0))); a rect's is a0' + u (a1' -
 * a0'), b0' + v (b1' - b0'), k' on its axes; then the previous transform values
 * are applied forward in the chain's order.  A miss (prim == 0, or a prim beyond
 * the world's list) gets three zeros.  With both arrays NULL the output is the
 * record's p bit for bit.  One kernel launch, asynchronous on `stream`; the
 * device's bytes are the host form's.  RTW_EINVAL for null pointers, buffers not
 * 8-byte aligned, n > 2^31, a non-finite time; n == 0 launches nothing. */
int rtw_world_prev_points_device(rtw_world w, const rtw_hit *d_hits, uint64_t n, double time,
                                 const double *d_a_prev, const double *d_xv_prev,
                                 double *d_prev_p, void *stream);
int rtw_world_prev_points_host(const rtw_world_desc *desc, const rtw_hit *hits, uint64_t n, double time,
                               const double *a_prev, const double *xv_prev, double *prev_p);

/* ---- mirror points ----
 * rtw_world_prev_points_device gives a mirror's own surface point, which stays
 * put (or moves with the mirror) while what the mirror reflects slides across
 * it.  These entries answer instead, for a record that counts as a mirror, WHICH
 * POINT OF THE MIRROR showed the same reflected thing in the previous frame: a
 * point M' on the mirror, with the mirror's own prim and its real depth under
 * cam_prev, so rtw_temporal_device and rtw_temporal_clamped_device take the
 * result as their d_prev_p and nothing else changes.
 *
 * A record counts as a mirror iff its prim is of the world's list, front == 1 and
 * the primitive's material is RTW_WMAT_METAL (any fuzz).  Its reflected ray has
 * origin p, direction d - 2 dot(d, n) n (the ray's unnormalised d, the record's
 * normal), the ray's time, t_min 0.001, t_max +inf.  With Mg = the record's
 * previous point (rtw_world_prev_points_*, at the ray's time), ng = its normal
 * under the previous numbers, O' = cam_prev's origin and the target S' = the
 * previous point of the reflected ray's hit (or, if it missed, the reflected unit
 * direction: the sky does not move):
 *   rect:   M' is where the line from O' to the target's mirror image across the
 *           plane (Mg, ng) meets that plane (exact);
 *   sphere: a thin-lens predictor (curvature (1 / cos + cos) / r') picks a start,
 *           then `steps` guarded Newton steps minimise |M - O'| + |M - S'| over the
 *           sphere of the previous numbers; a step is taken only if it is finite,
 *           the Hessian's determinant is > 0, the new normal faces the camera and
 *           the target, and the tangential residual shrank.
 * The result is Mg's bytes (rtw_world_prev_points_*'s) whenever the camera is not
 * in front of the tangent plane, an input or the result is not finite, the radius
 * is not > 0, the predictor's denominator is not > 0, a rect's target is not in
 * front of its plane or the plane's denominator is 0.  The exact expressions:
 * csrc/rtw_specular.hpp.  One specular bounce: a mirror seen in a mirror is
 * followed to the second mirror's surface; no occlusion test between M' and S'.
 *
 * Non-mirror records and misses get rtw_world_prev_points_device's bytes with
 * the record's ray's time.  Both previous arrays NULL: "the world stood still,
 * the camera may not have" — non-mirror records get p, M' is computed against
 * the current numbers.
 *
 * Device form: one launch on `stream`, no workspace, no readback, no atomics,
 * graph-capturable; equal inputs give equal bytes.  The reflected rays are walked
 * by the ray queries' own walks, chosen as rtw_world_trace_device chooses them
 * for this world (linear loop, union walk, per-lane walk with lane regeneration).
 * d_hits2 (optional, n x rtw_hit): the reflected ray's hit record, 80 zero bytes
 * for a non-mirror record or a reflected miss.  RTW_EINVAL for a NULL world,
 * cam_prev, d_rays, d_hits or d_prev_p, a world of another device, buffers not
 * 8-byte aligned, n > 2^31, steps > 8, unknown flags, an output that overlaps an
 * input or the other output (byte ranges).  n == 0 launches nothing.
 *
 * Host forms (the library has no host tracer): rtw_world_mirror_rays_host gives
 * the reflected rays and a byte per record (non-mirror records: 72 zero bytes);
 * the caller traces them (rtw_world_trace) and rtw_world_mirror_points_host takes
 * their hit records as hits2.  The device's bytes are this pipeline's. */
#define RTW_MIRROR_PREDICT_ONLY 1u /* flags bit 0: the predictor alone, no Newton step */
typedef struct {     /* every field 0 = its default */
  uint32_t steps;    /* Newton steps: 0 = 2; 1..8 */
  uint32_t flags;    /* RTW_MIRROR_PREDICT_ONLY */
} rtw_mirror_opts;   /* 8 bytes */
int rtw_world_mirror_points_device(rtw_world w, const rtw_ray *d_rays, const rtw_hit *d_hits, uint64_t n,
                                   const rtw_camera *cam_prev, const double *d_a_prev, const double *d_xv_prev,
                                   const rtw_mirror_opts *opts, double *d_prev_p, rtw_hit *d_hits2, void *stream);
int rtw_world_mirror_rays_host(const rtw_world_desc *desc, const rtw_ray *rays, const rtw_hit *hits, uint64_t n,
                               rtw_ray *rays2, uint8_t *is_mirror);
int rtw_world_mirror_points_host(const rtw_world_desc *desc, const rtw_ray *rays, const rtw_hit *hits,
                                 const rtw_hit *hits2, uint64_t n, const rtw_camera *cam_prev,
                                 const double *a_prev, const double *xv_prev, const rtw_mirror_opts *opts,
                                 double *prev_p);

#ifdef __cplusplus
}
#endif
#endif /* RTW_HIP_H */
