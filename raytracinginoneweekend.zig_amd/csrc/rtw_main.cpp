// rtw_main.cpp — command-line renderer: the reference's main() (main.zig:295-405)
// with the render loop replaced by the GPU (rtw_render for the cover scene's
// megakernel, rtw_world_render for every other scene).  Writes PPM (the
// reference writes PNG via zigimg; the pixel bytes are identical, main.zig:396).
//   rtw_render [--scene 1..7] [--width W] [--aspect A|W:H] [--spp N] [--depth D]
//              [--seed S] [--precision f64|f32] [--engine megakernel|wavefront]
//              [--chunk C] [--image earth.png] [--out out.ppm]
//              [--pass-spp N [--preview-dir DIR] [--max-noise X]
//                            [--pixel-noise X [--min-spp N] [--spp-map FILE]]]
//              [--denoise [--denoise-levels N] [--denoise-spatial]]
//              [--pick X,Y] [--focus-at X,Y]
//              [--frames N [--orbit DEG] [--rebuild-above R]
//                          [--temporal [--temporal-history M] [--denoise ...]
//                                      [--temporal-clamp G [--temporal-clamp-radius R]]
//                                      [--temporal-mirror [--temporal-mirror-steps K]]]]
//              [--aov-dir DIR]
// --aov-dir DIR writes the frame's feature buffers as two more images, DIR/albedo.ppm
// and DIR/normal.ppm (with --frames one pair per frame, albedo_%04d.ppm and
// normal_%04d.ppm): the guides of the frame's feature rays (rtw_hip.h "Guides"), read
// off their first hits by rtw_world_surface_device.  Albedo: each
// f32 channel a is quantised as a render quantises a linear colour,
// byte = (uint8)(256 * max(0, min(sqrt(a), 0.999))) in f64.  Normal: each component
// n goes through the same quantiser without the gamma,
// byte = (uint8)(256 * max(0, min(0.5 * (n + 1), 0.999))); a miss (normal 0,0,0) is
// mid-grey and its albedo the background.  Without the option nothing changes.
// --pick X,Y traces the feature ray of pixel (X, image row Y) (rtw_pixel_ray,
// rtw_world_trace) and prints one line,
//   pick x=.. y=.. prim=.. t=.. p=..,..,.. front=.. material=<kind>   (or: pick x=.. y=.. miss)
// with prim = the primitive's list index + 1, then exits without rendering.
// --focus-at X,Y renders with the camera focused on what that pixel shows: the
// focus distance is the depth of the pixel's hit along the view axis,
// dot(p - look_from, unit(look_at - look_from)), printed as focus_dist=..
// before the render; a pixel whose ray misses is an error.
// --pass-spp N renders the frame progressively, N samples per pass (a multiple
// of the chunk): the same --out bytes as without it.  --preview-dir DIR writes
// the image after every pass to DIR/pass_NNNN.ppm; --max-noise X stops once the
// frame's noise estimate (rtw_accum_noise) is <= X and prints the samples used.
// --pixel-noise X samples adaptively: a pixel stops once the standard error of
// its mean luminance is <= X (and it holds --min-spp samples), the run ends
// when every pixel has stopped or at --spp, and each pixel of --out is the
// one-shot render's with that pixel's own sample count; --spp-map FILE writes
// the counts as a binary PGM (8-bit, or 16-bit when a count exceeds 255).
// --denoise writes the feature-guided denoiser's image to --out
// and to every preview of --preview-dir: the guides are computed once per run,
// the frame goes through the accumulator (as one pass of --spp samples without
// --pass-spp) and is filtered with --denoise-levels N iterations (1-6, default
// 5).  --denoise-spatial (RTW_DENOISE_SPATIAL_VAR, §14.6) estimates the
// variance of pixels that hold fewer than two chunks from the image itself: the
// way to denoise a first preview of a single chunk.  Without --denoise the
// output bytes are unchanged, and without --denoise-spatial --denoise's are.
// --frames N --orbit DEG uploads the world once and updates it in place per
// frame (frame_%04d.ppm next to --out).  --rebuild-above R: after a frame's
// update, when the tree cost (rtw_world_bvh_cost) exceeds R times its value
// right after the creation or the last rebuild, the frame's numbers go through
// rtw_world_rebuild; one stderr line per rebuild gives the frame and the cost
// before and after.  The frames' bytes do not depend on it.
// --temporal (with --frames) accumulates the frames over time:
// frame k renders with seed S + k, its first hits are followed back into frame
// k - 1 and blended with what was seen there (at most --temporal-history M
// frames, default 32); each frame_%04d.ppm is the accumulated image, and with
// --denoise the denoiser's image of it, steered by the temporal variance
// (--denoise-spatial still fills the pixels whose history is too short for one).
// --temporal-clamp G clamps the history to the frame's neighbourhood before the
// blend: each channel to the mean +- G sigma of the current
// frame's (2R+1)^2 window around the pixel (G = 0: the default gamma;
// --temporal-clamp-radius R, 1-3, default 1).  Frame 0 has no history and keeps
// its bytes.  Without --temporal every run and every refusal is unchanged, and
// without --temporal-clamp every frame's bytes are.
// --temporal-mirror reprojects a metal surface from where it showed the same
// reflected thing in the last frame, not from its own surface point (DESIGN.md
// §21: rtw_world_mirror_points_device in place of rtw_world_prev_points_device;
// --temporal-mirror-steps K, 1-8 Newton steps, default 2).  Without the flag
// every frame's bytes are as before.
// Defaults are the reference's: scene 6 (main.zig:313) with that scene's own
// size, spp, camera and background (main.zig:316-362); --width/--aspect/--spp
// override them.  Scenes 4 and 7 need --image (assets/sekaichizu.png).
#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rtw_host.hpp"
#include "rtw_orbit.hpp"

static double parse_aspect(const char* s) {
  const char* c = std::strchr(s, ':');
  if (c) return std::atof(s) / std::atof(c + 1);
  return std::atof(s);
}

static bool parse_pixel(const char* s, uint32_t xy[2]) {
  char* e = nullptr;
  const unsigned long x = std::strtoul(s, &e, 10);
  if (e == s || *e != ',') return false;
  const char* s2 = e + 1;
  const unsigned long y = std::strtoul(s2, &e, 10);
  if (e == s2 || *e != 0) return false;
  xy[0] = (uint32_t)x, xy[1] = (uint32_t)y;
  return true;
}

static uint32_t be32(const unsigned char* p) { return (uint32_t)p[0] << 24 | p[1] << 16 | p[2] << 8 | p[3]; }

// 8-bit non-interlaced PNG -> RGBA8 (what zigimg hands texture.zig:133-140 for
// an RGBA file; grey / RGB / palette are expanded to RGBA).
static std::shared_ptr<rtw::Image> loadPNG(const std::string& path) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw rtw::Error(RTW_EINVAL, "cannot open " + path);
  std::vector<unsigned char> d;
  unsigned char buf[65536];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + n);
  std::fclose(f);
  if (d.size() < 8 || std::memcmp(d.data(), "\x89PNG\r\n\x1a\n", 8) != 0) throw rtw::Error(RTW_EINVAL, path + ": not a PNG");
  uint32_t w = 0, h = 0;
  int depth = 0, ctype = 0, interlace = 0;
  std::vector<unsigned char> idat, plte, trns;
  for (size_t i = 8; i + 12 <= d.size();) {
    const uint32_t len = be32(&d[i]);
    const std::string typ(reinterpret_cast<const char*>(&d[i + 4]), 4);
    const unsigned char* body = &d[i + 8];
    if (typ == "IHDR") {
      w = be32(body), h = be32(body + 4), depth = body[8], ctype = body[9], interlace = body[12];
    } else if (typ == "PLTE") {
      plte.assign(body, body + len);
    } else if (typ == "tRNS") {
      trns.assign(body, body + len);
    } else if (typ == "IDAT") {
      idat.insert(idat.end(), body, body + len);
    } else if (typ == "IEND") {
      break;
    }
    i += 12 + len;
  }
  if (depth != 8 || interlace != 0) throw rtw::Error(RTW_UNSUPPORTED, path + ": only 8-bit non-interlaced PNGs");
  const int ch = ctype == 6 ? 4 : ctype == 2 ? 3 : ctype == 4 ? 2 : 1;
  const size_t stride = (size_t)w * ch;
  std::vector<unsigned char> raw((stride + 1) * h);
  uLongf rl = (uLongf)raw.size();
  if (uncompress(raw.data(), &rl, idat.data(), (uLong)idat.size()) != Z_OK || rl != raw.size())
    throw rtw::Error(RTW_EINVAL, path + ": bad image data");
  std::vector<unsigned char> px(stride * h), prev(stride, 0);
  for (uint32_t y = 0; y < h; ++y) {  // scanline filters (PNG spec section 9)
    const unsigned char ft = raw[y * (stride + 1)];
    const unsigned char* line = &raw[y * (stride + 1) + 1];
    unsigned char* cur = &px[y * stride];
    for (size_t x = 0; x < stride; ++x) {
      const int a = x >= (size_t)ch ? cur[x - ch] : 0, b = prev[x], c = x >= (size_t)ch ? prev[x - ch] : 0;
      int pred = 0;
      if (ft == 1) pred = a;
      else if (ft == 2) pred = b;
      else if (ft == 3) pred = (a + b) >> 1;
      else if (ft == 4) {
        const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
      }
      cur[x] = (unsigned char)(line[x] + pred);
    }
    std::memcpy(prev.data(), cur, stride);
  }
  auto im = std::make_shared<rtw::Image>();
  im->width = w, im->height = h;
  im->rgba.resize((size_t)w * h * 4);
  for (size_t i = 0; i < (size_t)w * h; ++i) {
    unsigned char* o = &im->rgba[4 * i];
    const unsigned char* s = &px[ch * i];
    if (ctype == 6) std::memcpy(o, s, 4);
    else if (ctype == 2) o[0] = s[0], o[1] = s[1], o[2] = s[2], o[3] = 255;
    else if (ctype == 4) o[0] = o[1] = o[2] = s[0], o[3] = s[1];
    else if (ctype == 0) o[0] = o[1] = o[2] = s[0], o[3] = 255;
    else {
      o[0] = plte[3 * s[0]], o[1] = plte[3 * s[0] + 1], o[2] = plte[3 * s[0] + 2];
      o[3] = s[0] < trns.size() ? trns[s[0]] : 255;
    }
  }
  return im;
}

// --aov-dir: the two images of a frame's guides (the rules: this file's header comment); k < 0: a single frame.
static uint8_t quantise_unit(double x) { return (uint8_t)(256.0 * std::fmax(0.0, std::fmin(x, 0.999))); }
static void writeAovs(const std::string& dir, int k, const std::vector<rtw_guide>& g, uint32_t w, uint32_t h) {
  std::vector<uint8_t> albedo(g.size() * 3), normal(g.size() * 3);
  for (size_t i = 0; i < g.size(); ++i)
    for (int c = 0; c < 3; ++c) {
      albedo[3 * i + c] = quantise_unit(std::sqrt((double)g[i].albedo[c]));
      normal[3 * i + c] = quantise_unit(0.5 * ((double)g[i].normal[c] + 1.0));
    }
  char suffix[32] = "";
  if (k >= 0) std::snprintf(suffix, sizeof(suffix), "_%04d", k);
  rtw::writePPM(dir + "/albedo" + suffix + ".ppm", albedo, w, h);
  rtw::writePPM(dir + "/normal" + suffix + ".ppm", normal, w, h);
}

int main(int argc, char** argv) {
  uint32_t scene = 6;  // main.zig:313
  uint32_t width = 0, spp = 0, depth = 50, chunk = 0, precision = RTW_PRECISION_F64, engine = RTW_ENGINE_MEGAKERNEL;
  uint32_t pass_spp = 0, min_spp = 0, frames = 1;
  double orbit = 0, rebuild_above = -1.0;  // (< 0: never rebuild)
  double aspect = 0, max_noise = 0, pixel_noise = 0;
  uint64_t seed = 42;
  std::string out = "out.ppm", image_path, preview_dir, spp_map, aov_dir;
  bool denoise = false, denoise_spatial = false, temporal = false;
  uint32_t denoise_levels = 0, temporal_history = 0, temporal_clamp_radius = 0;
  bool temporal_clamp = false, temporal_clamp_radius_set = false;
  double temporal_clamp_gamma = 0;
  bool temporal_mirror = false, temporal_mirror_steps_set = false;
  uint32_t temporal_mirror_steps = 0;
  bool pick = false, focus_at = false;
  uint32_t pick_xy[2] = {0, 0}, focus_xy[2] = {0, 0};
  for (int i = 1; i < argc; i += 2) {
    const std::string k = argv[i];
    if (k == "--denoise" || k == "--denoise-spatial" || k == "--temporal" || k == "--temporal-mirror") {  // (the options without a value)
      (k == "--denoise" ? denoise : k == "--temporal" ? temporal : k == "--temporal-mirror" ? temporal_mirror : denoise_spatial) = true;
      --i;
      continue;
    }
    if (i + 1 >= argc) break;
    const char* v = argv[i + 1];
    if (k == "--scene") scene = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (k == "--width") width = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (k == "--aspect") aspect = parse_aspect(v);
    else if (k == "--spp") spp = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (k == "--depth") depth = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (k == "--seed") seed = std::strtoull(v, nullptr, 10);
    else if (k == "--precision") precision = std::string(v) == "f32" ? RTW_PRECISION_F32 : RTW_PRECISION_F64;
    else if (k == "--engine") engine = std::string(v) == "wavefront" ? RTW_ENGINE_WAVEFRONT : RTW_ENGINE_MEGAKERNEL;
    else if (k == "--chunk") chunk = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (k == "--image") image_path = v;
    else if (k == "--out") out = v;
    else if (k == "--pass-spp") pass_spp = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (k == "--preview-dir") preview_dir = v;
    else if (k == "--max-noise") max_noise = std::atof(v);
    else if (k == "--pixel-noise") pixel_noise = std::atof(v);
    else if (k == "--min-spp") min_spp = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (k == "--spp-map") spp_map = v;
    else if (k == "--aov-dir") aov_dir = v;
    else if (k == "--frames") frames = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (k == "--orbit") orbit = std::atof(v);
    else if (k == "--rebuild-above") rebuild_above = std::atof(v);
    else if (k == "--temporal-history") temporal_history = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (k == "--temporal-clamp") temporal_clamp = true, temporal_clamp_gamma = std::atof(v);
    else if (k == "--temporal-mirror-steps") {
      temporal_mirror_steps_set = true, temporal_mirror_steps = (uint32_t)std::strtoul(v, nullptr, 10);
    } else if (k == "--temporal-clamp-radius") {
      temporal_clamp_radius_set = true, temporal_clamp_radius = (uint32_t)std::strtoul(v, nullptr, 10);
    }
    else if (k == "--denoise-levels") denoise_levels = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (k == "--pick" || k == "--focus-at") {
      const bool is_pick = k == "--pick";
      if (!parse_pixel(v, is_pick ? pick_xy : focus_xy)) {
        std::fprintf(stderr, "%s needs X,Y\n", k.c_str());
        return 2;
      }
      (is_pick ? pick : focus_at) = true;
    }
    else {
      std::fprintf(stderr, "unknown option %s\n", k.c_str());
      return 2;
    }
  }
  if (pass_spp == 0 && (!preview_dir.empty() || max_noise > 0 || pixel_noise > 0)) {
    std::fprintf(stderr, "--preview-dir, --max-noise and --pixel-noise need --pass-spp\n");
    return 2;
  }
  if ((denoise_levels || denoise_spatial) && !denoise) {
    std::fprintf(stderr, "--denoise-levels and --denoise-spatial need --denoise\n");
    return 2;
  }
  if (temporal_history && !temporal) {
    std::fprintf(stderr, "--temporal-history needs --temporal\n");
    return 2;
  }
  if ((temporal_clamp || temporal_clamp_radius_set) && !temporal) {
    std::fprintf(stderr, "--temporal-clamp and --temporal-clamp-radius need --temporal\n");
    return 2;
  }
  if ((temporal_mirror || temporal_mirror_steps_set) && !temporal) {
    std::fprintf(stderr, "--temporal-mirror and --temporal-mirror-steps need --temporal\n");
    return 2;
  }
  if (temporal_mirror_steps_set && (!temporal_mirror || temporal_mirror_steps < 1 || temporal_mirror_steps > 8)) {
    std::fprintf(stderr, "--temporal-mirror-steps needs --temporal-mirror and K in 1..8\n");
    return 2;
  }
  if (temporal_clamp_radius_set && !temporal_clamp) {
    std::fprintf(stderr, "--temporal-clamp-radius needs --temporal-clamp\n");
    return 2;
  }
  if (temporal_clamp && (!(temporal_clamp_gamma >= 0 && temporal_clamp_gamma < 1e30) ||
                         (temporal_clamp_radius_set && (temporal_clamp_radius < 1 || temporal_clamp_radius > 3)))) {
    std::fprintf(stderr, "--temporal-clamp needs a finite G >= 0 (0: the default) and --temporal-clamp-radius R in 1..3\n");
    return 2;
  }
  if (temporal && (frames < 2 || pass_spp || pick || focus_at || temporal_history > 4096)) {
    std::fprintf(stderr, "--temporal needs --frames N with N >= 2 (no --pass-spp, --pick, --focus-at) and M <= 4096\n");
    return 2;
  }
  if (frames == 0 || (frames > 1 && (pass_spp || (denoise && !temporal) || pick || focus_at))) {
    std::fprintf(stderr, "--frames needs N >= 1 and renders one-shot frames (no --pass-spp, --denoise, --pick, --focus-at)\n");
    return 2;
  }
  if (rebuild_above != -1.0 && (frames < 2 || !(rebuild_above >= 0))) {
    std::fprintf(stderr, "--rebuild-above needs R >= 0 and --frames N with N >= 2\n");
    return 2;
  }
  if (!(pixel_noise > 0) && (min_spp || !spp_map.empty())) {
    std::fprintf(stderr, "--min-spp and --spp-map need --pixel-noise\n");
    return 2;
  }
  try {
    const rtw_scene_settings st = rtw::sceneSettings(scene);  // main.zig:303-362
    const double asp = aspect > 0 ? aspect : st.aspect;
    const uint32_t W = width ? width : st.width;
    const uint32_t H = (width || aspect > 0) ? rtw::imageHeight(W, asp) : st.height;
    const uint32_t S = spp ? spp : st.spp;
    auto camera = [&](double focus_dist) {
      return rtw::Camera::init({st.look_from[0], st.look_from[1], st.look_from[2]},
                               {st.look_at[0], st.look_at[1], st.look_at[2]}, {0, 1, 0}, st.vfov, asp, st.aperture,
                               focus_dist, 0, 1);  // main.zig:366-376
    };
    rtw::Camera cam = camera(10.0);
    rtw::Random rng = rtw::Random::init(seed);  // main.zig:300-301
    std::shared_ptr<rtw::Image> earth;
    if (scene == 4 || scene == 7) {
      if (image_path.empty()) throw rtw::Error(RTW_EINVAL, "scenes 4 and 7 need --image assets/sekaichizu.png");
      earth = loadPNG(image_path);
    }
    rtw::Hittable world;
    switch (scene) {
      case 1: world = rtw::generateRandomScene(rng); break;
      case 2: world = rtw::generateTwoSpheres(rng); break;
      case 3: world = rtw::generateTwoPerlinSpheres(rng); break;
      case 4: world = rtw::generateEarthScene(earth); break;
      case 5: world = rtw::generateSimpleLightScene(rng); break;
      case 6: world = rtw::generateCornellBox(); break;
      case 7: world = rtw::generateGlobeScene(rng, earth); break;
      default: throw rtw::Error(RTW_EINVAL, "scene must be 1..7");
    }
    if (pick || focus_at) {
      // The closest hit of the pixel's feature ray (the guides' ray, rtw_hip.h) over the flattened world.
      const rtw::FlatWorld fw = rtw::flattenWorld(world);
      const rtw_world_desc desc = fw.desc();
      auto trace_pixel = [&](const uint32_t xy[2], rtw_hit& h) {
        const rtw_camera c = cam.to_c();
        rtw_ray r;
        if (rtw_pixel_ray(&c, W, H, xy[0], xy[1], &r) != RTW_OK)
          throw rtw::Error(RTW_EINVAL, "pixel " + std::to_string(xy[0]) + "," + std::to_string(xy[1]) + " is outside the " +
                                           std::to_string(W) + "x" + std::to_string(H) + " image");
        rtw_world w = nullptr;
        int rc = rtw_world_create(&desc, 0, &w);
        if (rc == RTW_OK) rc = rtw_world_trace(w, &r, 1, nullptr, &h);
        rtw_world_destroy(w);
        if (rc != RTW_OK) throw rtw::Error(rc, rtw_last_error());
      };
      rtw_hit h;
      if (pick) {
        trace_pixel(pick_xy, h);
        if (h.prim == 0) {
          std::printf("pick x=%u y=%u miss\n", pick_xy[0], pick_xy[1]);
        } else {
          static const char* const kinds[] = {"lambert", "metal", "dielectric", "light"};
          const uint32_t mk = desc.mats[desc.prims[h.prim - 1].mat].kind;
          std::printf("pick x=%u y=%u prim=%u t=%.17g p=%.17g,%.17g,%.17g front=%u material=%s\n", pick_xy[0], pick_xy[1],
                      h.prim, h.t, h.p[0], h.p[1], h.p[2], h.front, mk < 4 ? kinds[mk] : "unknown");
        }
        return 0;
      }
      trace_pixel(focus_xy, h);
      if (h.prim == 0)
        throw rtw::Error(RTW_EINVAL, "--focus-at " + std::to_string(focus_xy[0]) + "," + std::to_string(focus_xy[1]) +
                                         ": the pixel's ray hits nothing to focus on");
      double a[3], len2 = 0;
      for (int k = 0; k < 3; ++k) a[k] = st.look_at[k] - st.look_from[k], len2 += a[k] * a[k];
      const double len = std::sqrt(len2);
      for (int k = 0; k < 3; ++k) a[k] = a[k] / len;
      const double f = (h.p[0] - st.look_from[0]) * a[0] + (h.p[1] - st.look_from[1]) * a[1] +
                       (h.p[2] - st.look_from[2]) * a[2];
      std::printf("focus_dist=%.17g\n", f);
      std::fflush(stdout);
      cam = camera(f);
    }
    std::vector<uint8_t> rgb((size_t)W * H * 3);
    uint32_t used = S;
    std::vector<uint32_t> counts;
    rtw::AdaptiveOpts adaptive;
    adaptive.pixel_noise = pixel_noise, adaptive.min_spp = min_spp, adaptive.counts = &counts;
    rtw_denoise_opts dn;
    std::memset(&dn, 0, sizeof(dn));
    dn.levels = denoise_levels;
    if (denoise_spatial) dn.flags |= RTW_DENOISE_SPATIAL_VAR;
    if (denoise && pass_spp == 0 && !temporal) pass_spp = S;  // the whole frame as one pass of the accumulator
    if (denoise && !temporal) {
      // The colour term needs a variance, and the variance two full chunks (without it the
      // filter blurs what no guide describes — reflections, shadows — and a 20-spp preview gets worse).
      const uint32_t c = std::min(chunk ? chunk : RTW_DEFAULT_CHUNK, S);
      if (std::min(pass_spp, S) / c < 2 && denoise_spatial)
        std::fprintf(stderr,
                     "note: the first image holds fewer than two chunks of %u samples; its variance is estimated from the "
                     "image itself (--denoise-spatial)\n", c);
      else if (std::min(pass_spp, S) / c < 2)
        std::fprintf(stderr,
                     "note: the first image holds fewer than two chunks of %u samples, so its variance is unknown and the "
                     "denoiser's colour term is off for it; --chunk %u gives it one, or --denoise-spatial estimates it "
                     "from the image\n", c, std::max(1u, std::min(pass_spp, S) / 2));
    }
    // --pass-spp: the frame through the accumulator, a preview per pass
    auto progressive = [&](const rtw_params& p, const rtw::FlatScene* fs, const rtw_world_desc* wd) {
      if (!preview_dir.empty()) (void)mkdir(preview_dir.c_str(), 0777);  // (an existing directory is fine)
      const rtw_camera c = cam.to_c();
      return rtw::renderProgressive(c, p, pass_spp, fs, wd, max_noise,
                                    [&](const rtw::PassInfo& i, const std::vector<uint8_t>& img) {
                                      if (preview_dir.empty()) return;
                                      char name[32];
                                      std::snprintf(name, sizeof(name), "/pass_%04u.ppm", i.pass);
                                      rtw::writePPM(preview_dir + name, img, W, H);
                                    },
                                    &used, pixel_noise > 0 ? &adaptive : nullptr, denoise ? &dn : nullptr);
    };
    rtw_params p;
    std::memset(&p, 0, sizeof(p));
    p.width = W, p.height = H, p.spp = S, p.max_depth = depth, p.seed = seed;
    for (int k = 0; k < 3; ++k) p.background[k] = st.background[k];
    p.row_begin = 0, p.row_stride = 1, p.row_count = H, p.chunk = chunk, p.device = -1;
    if (frames > 1) {
      // --frames N --orbit DEG: one upload, an in-place update per frame (rtw_hip.h "dynamic worlds");
      // frame_0000.ppm ... next to --out, the last frame in --out itself
      const rtw::FlatWorld fw = rtw::flattenWorld(world);
      const rtw_world_desc desc = fw.desc();
      p.precision = RTW_PRECISION_F64, p.engine = RTW_ENGINE_MEGAKERNEL;
      const size_t slash = out.find_last_of('/');
      const std::string dir = slash == std::string::npos ? "" : out.substr(0, slash + 1);
      const rtw::FrameFn write_frame = [&](uint32_t k, const std::vector<uint8_t>& img) {
        char name[32];
        std::snprintf(name, sizeof(name), "frame_%04u.ppm", k);
        rtw::writePPM(dir + name, img, W, H);
        rgb = img;
      };
      rtw::GuideFn write_guides;  // (empty without --aov-dir: the frames then compute nothing for it)
      if (!aov_dir.empty()) {
        (void)mkdir(aov_dir.c_str(), 0777);  // (an existing directory is fine)
        write_guides = [&](uint32_t k, const std::vector<rtw_guide>& g) { writeAovs(aov_dir, (int)k, g, W, H); };
      }
      if (temporal) {
        rtw::TemporalRun run;
        run.max_history = temporal_history, run.denoise = denoise, run.dn = dn;
        rtw_temporal_clamp tc{};
        tc.gamma = temporal_clamp_gamma, tc.radius = temporal_clamp_radius;
        rtw_mirror_opts mo{};
        mo.steps = temporal_mirror_steps;
        rtw::renderOrbitTemporal(cam.to_c(), p, desc, frames, orbit, write_frame, run, rebuild_above, write_guides,
                                 temporal_clamp ? &tc : nullptr, temporal_mirror ? &mo : nullptr);
      } else {
        rtw::renderOrbit(cam.to_c(), p, desc, frames, orbit, write_frame, rebuild_above, write_guides);
      }
    } else if (scene == 1 && pass_spp) {
      p.precision = precision, p.engine = engine;
      const rtw::FlatScene fs = rtw::flatten(world);
      rgb = progressive(p, &fs, nullptr);
    } else if (scene == 1) {  // the cover scene: the sphere megakernel (or the wavefront engine)
      rtw::RenderSettings rs;
      rs.width = W, rs.aspect_ratio = asp, rs.samples_per_pixel = S, rs.max_depth = depth, rs.seed = seed;
      rs.precision = precision, rs.chunk = chunk, rs.engine = engine;
      rs.background = {st.background[0], st.background[1], st.background[2]};
      rgb = rtw::render(cam, world, rs, H);  // main.zig:378-402
    } else {
      const rtw::FlatWorld fw = rtw::flattenWorld(world);
      const rtw_world_desc desc = fw.desc();
      p.precision = RTW_PRECISION_F64, p.engine = RTW_ENGINE_MEGAKERNEL;
      if (pass_spp) {
        rgb = progressive(p, nullptr, &desc);
      } else {
        const rtw_camera c = cam.to_c();
        const int rc = rtw_world_render(&c, &desc, &p, rgb.data(), nullptr);  // main.zig:378-402
        if (rc != RTW_OK) throw rtw::Error(rc, rtw_last_error());
      }
    }
    rtw::writePPM(out, rgb, W, H);  // main.zig:405
    if (!aov_dir.empty() && frames == 1) {  // (with --frames the frames wrote theirs)
      (void)mkdir(aov_dir.c_str(), 0777);
      const rtw::FlatWorld fw = rtw::flattenWorld(world);
      writeAovs(aov_dir, -1, rtw::frameGuides(cam.to_c(), W, H, st.background, fw.desc()), W, H);
    }
    if (max_noise > 0) std::fprintf(stderr, "noise budget %g: %u of %u samples used\n", max_noise, used, S);
    if (pixel_noise > 0) {
      uint64_t total = 0;
      for (uint32_t c : counts) total += c;
      std::fprintf(stderr, "pixel noise budget %g: %.2f samples per pixel on average, %u at most\n", pixel_noise,
                   (double)total / (double)counts.size(), used);
      if (!spp_map.empty()) rtw::writeCountsPGM(spp_map, counts, W, H);
    }
    std::fprintf(stderr, "wrote %s (scene %u, %ux%u, %u spp)\n", out.c_str(), scene, W, H, used);
  } catch (const rtw::Error& e) {
    std::fprintf(stderr, "rtw_render: %s (status %d)\n", e.what(), e.status);
    return 1;
  }
  return 0;
}
