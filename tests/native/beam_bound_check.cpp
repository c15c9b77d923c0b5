// beam_bound_check — the tile-beam bound (csrc/rtw_beam.hpp) is conservative:
// for every 8x8 tile of a frame, rays made by Camera.getRay's formulas
// (main.zig:91-100, :390-391) at the extremes of the tile's parameters — jitter
// 0 and 1 - ulp, lens points on the unit circle and at 0, both shutter ends —
// and at seeded random values are solved exactly (f64, Sphere.hit /
// MovingSphere.hit, hittable.zig:95-131, :165-201) against every sphere; a
// sphere with a root >= tmin must be in the tile's mask.
//   beam_bound_check <scene.txt> [popcount]
//   beam_bound_check <scene.txt> cases <cases.txt> [quick]
//   beam_bound_check <scene.txt> masks <cases.txt>
// scene.txt: n, then per sphere "c0.xyz c1.xyz radius t0 t1 moving".
// `popcount`: also print the mean mask popcount of the narrow spheres over the
// 1200x675 frame's tiles with the cover camera.
// cases.txt: n, then per case the raw rtw_camera fields "origin.xyz
// horizontal.xyz vertical.xyz lower_left_corner.xyz u.xyz v.xyz lens_radius
// time0 time1" (any struct: it need not come from Camera.init) and the frame
// "W H row_begin row_stride row_count" (the kernel's tiles are cut from
// row_count rows, which may be fewer than the frame holds).
// `cases`: the rays above for every case instead of the built-in cameras, and
// for every (tile, sphere) pair the mask EXCLUDES rays aimed at that sphere:
// from the lens centre and 16 rim points, at both shutter ends and the middle,
// through the point of the tile's part of the focus plane nearest to the line
// lens point -> sphere centre (a sphere behind the lens: the point mirrored
// through the tile's centre); any hit is a violation.  Also prints "pairs P
// in_mask M tiles T full_tiles F neg_tiles G narrow_hits N aimed A": the narrow
// (tile, sphere) pairs and those in their mask, the tiles, those whose mask
// holds every narrow sphere / a narrow sphere of negative radius, the hits on
// narrow spheres, the aimed rays.  `quick`: stop after the first case with a
// violation.
// `masks`: no rays; per case "case i popcount P tiles T full F guarded G narrow
// N": the sum over tiles of the narrow spheres in the mask (what the
// megakernel counts per fetched batch, RTW_STAT primary_mask_popcount), the
// tiles whose mask is full, and those the wide-cone guard answers for.
// Narrow: radius < 100 (rtw_layout.hpp kWideRadius; a negative radius is narrow).
// Prints "rays R hits H violations V"; exit status 1 when V > 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rtw_beam.hpp"

namespace {

struct Sph {
  double c0[3], c1[3], r, t0, t1;
  int moving;
};
struct V {
  double x, y, z;
};
V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V operator*(V a, double t) { return {a.x * t, a.y * t, a.z * t}; }
double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
V unit(V a) { return a * (1.0 / std::sqrt(dot(a, a))); }

struct Cam {  // Camera.init (main.zig:60-89)
  V origin, llc, hor, ver, u, v;
  double lens_radius, time0, time1;
};
Cam cam_init(V from, V at, V vup, double vfov, double aspect, double aperture, double focus, double t0, double t1) {
  const double theta = vfov * M_PI / 180.0, hh = std::tan(theta / 2.0);
  const double vh = 2.0 * hh, vw = aspect * vh;
  Cam c;
  const V w = unit(from - at);
  c.u = unit(cross(vup, w));
  c.v = cross(w, c.u);
  c.origin = from;
  c.hor = c.u * (focus * vw);
  c.ver = c.v * (focus * vh);
  c.llc = c.origin - c.hor * 0.5 - c.ver * 0.5 - w * focus;
  c.lens_radius = aperture / 2.0;
  c.time0 = t0, c.time1 = t1;
  return c;
}

uint64_t g_rng = 0x243F6A8885A308D3ull;
double rnd() {  // xorshift64*, [0, 1)
  g_rng ^= g_rng >> 12, g_rng ^= g_rng << 25, g_rng ^= g_rng >> 27;
  return (double)((g_rng * 0x2545F4914F6CDD1Dull) >> 11) * 0x1p-53;
}

const double kTmin = 0.001;

bool exact_hit(const Sph& s, V o, V d, double time) {
  V c = {s.c0[0], s.c0[1], s.c0[2]};
  if (s.moving) {
    const double fr = (time - s.t0) / (s.t1 - s.t0);
    c = c + V{s.c1[0] - s.c0[0], s.c1[1] - s.c0[1], s.c1[2] - s.c0[2]} * fr;
  }
  const V oc = o - c;
  const double a = dot(d, d), hb = dot(oc, d), cc = dot(oc, oc) - s.r * s.r;
  const double disc = hb * hb - a * cc;
  if (disc < 0.0) return false;
  const double sq = std::sqrt(disc);
  double root = (-hb - sq) / a;
  if (root < kTmin) root = (-hb + sq) / a;
  return !(root < kTmin);
}

struct Totals {
  unsigned long long rays = 0, hits = 0, viol = 0, pop = 0, tiles = 0;
  unsigned long long pairs = 0, full = 0, neg = 0, guarded = 0, narrow_hits = 0, aimed = 0;
};

bool narrow(const Sph& s) { return !(s.r >= 100.0); }  // rtw_scene_pack.cpp: radius >= kWideRadius is wide

// x of M x = r (columns m0, m1, m2), Cramer's rule; false: singular.
bool solve3(V m0, V m1, V m2, V r, double x[3]) {
  const double det = dot(m0, cross(m1, m2));
  if (!(std::fabs(det) > 1e-300)) return false;
  x[0] = dot(r, cross(m1, m2)) / det;
  x[1] = dot(m0, cross(r, m2)) / det;
  x[2] = dot(m0, cross(m1, r)) / det;
  return std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]);
}

// One frame: every tile's mask; with `rays`, the exact solves against it; with `aimed`, also the rays aimed
// at the spheres a mask excludes.  rc: the rows rendered (row_count).
void run_frame(const std::vector<Sph>& S, const Cam& c, uint32_t W, uint32_t H, uint32_t rb, uint32_t rs, uint32_t rc,
               bool rays, bool aimed, Totals& T) {
  const double O[3] = {c.origin.x, c.origin.y, c.origin.z}, L[3] = {c.llc.x, c.llc.y, c.llc.z};
  const double Hh[3] = {c.hor.x, c.hor.y, c.hor.z}, Vv[3] = {c.ver.x, c.ver.y, c.ver.z};
  const double U[3] = {c.u.x, c.u.y, c.u.z}, Vu[3] = {c.v.x, c.v.y, c.v.z};
  const double one_m = std::nextafter(1.0, 0.0);
  std::vector<char> mask(S.size());
  for (uint32_t ty = 0; ty * 8 < rc; ++ty)
    for (uint32_t tx = 0; tx * 8 < W; ++tx) {
      const uint32_t px0 = tx * 8, px1 = std::min(px0 + 7, W - 1);
      const uint32_t ly0 = ty * 8, ly1 = std::min(ly0 + 7, rc - 1);
      const uint32_t y0 = rb + ly0 * rs, y1 = rb + ly1 * rs;
      const rtwb::Beam b = rtwb::tile_beam(O, L, Hh, Vv, U, Vu, c.lens_radius, W, H, px0, px1, y0, y1);
      for (size_t i = 0; i < S.size(); ++i) {
        const double dc[3] = {S[i].c1[0] - S[i].c0[0], S[i].c1[1] - S[i].c0[1], S[i].c1[2] - S[i].c0[2]};
        mask[i] = rtwb::beam_may_hit(b, S[i].c0, dc, S[i].r, S[i].moving != 0, S[i].t0, S[i].t1, c.time0, c.time1);
      }
      {
        unsigned nn = 0, in = 0, neg = 0;
        for (size_t i = 0; i < S.size(); ++i)
          if (narrow(S[i])) nn++, in += mask[i] ? 1 : 0, neg += (mask[i] && S[i].r < 0.0) ? 1 : 0;
        T.pop += in, T.pairs += nn, T.full += (nn > 0 && in == nn) ? 1 : 0, T.neg += neg ? 1 : 0;
        // the wide-cone guard answers for the tile: a speck far behind the lens is in its mask
        const double far[3] = {b.O[0] - 1e3 * b.D[0], b.O[1] - 1e3 * b.D[1], b.O[2] - 1e3 * b.D[2]}, z3[3] = {0, 0, 0};
        T.guarded += rtwb::beam_may_hit(b, far, z3, 1e-6, false, 0.0, 1.0, c.time0, c.time1) ? 1 : 0;
      }
      T.tiles++;
      if (!rays) continue;
      if (aimed) {
        const double w1 = (double)W - 1.0, h1 = (double)H - 1.0;
        const double sc = 0.5 * ((double)px0 + (double)px1 + 1.0) / w1;
        const double tc = 0.5 * ((double)(H - 1 - y1) + (double)(H - y0)) / h1;
        for (size_t i = 0; i < S.size(); ++i) {
          if (mask[i]) continue;
          for (int li = 0; li < 17; ++li) {
            const double ang = (li - 1) * (M_PI / 8.0);
            const double dx = li ? std::cos(ang) : 0.0, dy = li ? std::sin(ang) : 0.0;
            const V off = c.u * (dx * c.lens_radius) + c.v * (dy * c.lens_radius);
            const V o = c.origin + off;
            for (int ti = 0; ti < 3; ++ti) {
              const double time = ti == 0 ? c.time0 : (ti == 1 ? c.time1 : 0.5 * (c.time0 + c.time1));
              V cen = {S[i].c0[0], S[i].c0[1], S[i].c0[2]};
              if (S[i].moving)
                cen = cen + V{S[i].c1[0] - S[i].c0[0], S[i].c1[1] - S[i].c0[1], S[i].c1[2] - S[i].c0[2]} *
                                ((time - S[i].t0) / (S[i].t1 - S[i].t0));
              // llc + s hor + t ver = o + lam (cen - o)
              double x[3];
              if (!solve3(c.hor, c.ver, (cen - o) * -1.0, o - c.llc, x)) continue;
              double s = x[0], t = x[1];
              if (x[2] < 0.0) s = 2.0 * sc - s, t = 2.0 * tc - t;  // behind the lens: the far side of the tile
              // the tile's nearest pixel column and row, and the jitter in it
              const double sx = s * w1, jx = t * h1;
              uint32_t px = px0;
              if (sx > (double)px0) px = sx >= (double)px1 ? px1 : (uint32_t)sx;
              const double ju = std::fmin(std::fmax(sx - (double)px, 0.0), one_m);
              uint32_t jbest = H - 1 - (rb + ly0 * rs);
              double dbest = INFINITY;
              for (uint32_t ly = ly0; ly <= ly1; ++ly) {
                const uint32_t j = H - 1 - (rb + ly * rs);
                const double dist = jx < (double)j ? (double)j - jx : (jx > (double)j + 1.0 ? jx - ((double)j + 1.0) : 0.0);
                if (dist < dbest) dbest = dist, jbest = j;
              }
              const double jv = std::fmin(std::fmax(jx - (double)jbest, 0.0), one_m);
              const double u = ((double)px + ju) / w1, v = ((double)jbest + jv) / h1;
              const V d = c.llc + c.hor * u + c.ver * v - c.origin - off;
              T.aimed++;
              if (exact_hit(S[i], o, d, time)) {
                T.hits++;
                if (narrow(S[i])) T.narrow_hits++;
                if (T.viol < 5)
                  fprintf(stderr, "violation (aimed): %ux%u rows %u:%u:%u tile (%u, %u) pixel (%u, %u) sphere %zu\n", W, H,
                          rb, rs, rc, tx, ty, px, H - 1 - jbest, i);
                T.viol++;
              }
            }
          }
        }
      }
      for (uint32_t ly = ly0; ly <= ly1; ++ly)
        for (uint32_t px = px0; px <= px1; ++px) {
          const uint32_t y = rb + ly * rs, j = H - 1 - y;
          for (int ji = 0; ji < 6; ++ji) {
            const double ju = ji < 4 ? ((ji & 1) ? one_m : 0.0) : rnd(), jv = ji < 4 ? ((ji & 2) ? one_m : 0.0) : rnd();
            const double u = ((double)px + ju) / ((double)W - 1.0), v = ((double)j + jv) / ((double)H - 1.0);
            for (int li = 0; li < 6; ++li) {
              double dx = 0.0, dy = 0.0;
              if (li < 4) {  // on the unit circle: a random angle per quadrant
                const double ang = (li + rnd()) * (M_PI / 2.0);
                dx = std::cos(ang), dy = std::sin(ang);
              } else if (li == 5) {
                do dx = 2.0 * rnd() - 1.0, dy = 2.0 * rnd() - 1.0;
                while (dx * dx + dy * dy >= 1.0);
              }
              const V off = c.u * (dx * c.lens_radius) + c.v * (dy * c.lens_radius);
              const V o = c.origin + off;
              const V d = c.llc + c.hor * u + c.ver * v - c.origin - off;
              for (int ti = 0; ti < 3; ++ti) {
                const double tr = ti == 0 ? 0.0 : (ti == 1 ? one_m : rnd());
                const double time = c.time0 + tr * (c.time1 - c.time0);
                T.rays++;
                for (size_t i = 0; i < S.size(); ++i)
                  if (exact_hit(S[i], o, d, time)) {
                    T.hits++;
                    if (narrow(S[i])) T.narrow_hits++;
                    if (!mask[i]) {
                      if (T.viol < 5)
                        fprintf(stderr, "violation: %ux%u rows %u::%u tile (%u, %u) pixel (%u, %u) sphere %zu\n", W, H,
                                rb, rs, tx, ty, px, y, i);
                      T.viol++;
                    }
                  }
              }
            }
          }
        }
    }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  int n = 0;
  if (fscanf(f, "%d", &n) != 1 || n <= 0) return 2;
  std::vector<Sph> S(n);
  for (auto& s : S)
    if (fscanf(f, "%lf %lf %lf %lf %lf %lf %lf %lf %lf %d", &s.c0[0], &s.c0[1], &s.c0[2], &s.c1[0], &s.c1[1], &s.c1[2],
               &s.r, &s.t0, &s.t1, &s.moving) != 10)
      return 2;
  fclose(f);
  if (argc > 3 && (std::strcmp(argv[2], "cases") == 0 || std::strcmp(argv[2], "masks") == 0)) {
    const bool rays = std::strcmp(argv[2], "cases") == 0, quick = argc > 4 && std::strcmp(argv[4], "quick") == 0;
    FILE* cf = fopen(argv[3], "r");
    int nc = 0;
    if (!cf || fscanf(cf, "%d", &nc) != 1 || nc <= 0) return 2;
    Totals T;
    for (int i = 0; i < nc; ++i) {
      Cam c;
      V* const vs[6] = {&c.origin, &c.hor, &c.ver, &c.llc, &c.u, &c.v};
      for (V* v : vs)
        if (fscanf(cf, "%lf %lf %lf", &v->x, &v->y, &v->z) != 3) return 2;
      uint32_t W, H, rb, rs, rc;
      if (fscanf(cf, "%lf %lf %lf %u %u %u %u %u", &c.lens_radius, &c.time0, &c.time1, &W, &H, &rb, &rs, &rc) != 8)
        return 2;
      if (W < 2 || H < 2 || rs == 0 || rc == 0 || (uint64_t)rb + (uint64_t)(rc - 1) * rs >= H) return 2;
      if (rays) {
        run_frame(S, c, W, H, rb, rs, rc, true, true, T);
        if (quick && T.viol) break;
      } else {
        Totals P;
        run_frame(S, c, W, H, rb, rs, rc, false, false, P);
        printf("case %d popcount %llu tiles %llu full %llu guarded %llu narrow %llu\n", i, P.pop, P.tiles, P.full,
               P.guarded, P.tiles ? P.pairs / P.tiles : 0ull);
      }
    }
    fclose(cf);
    if (rays) {
      printf("rays %llu hits %llu violations %llu\n", T.rays, T.hits, T.viol);
      printf("pairs %llu in_mask %llu tiles %llu full_tiles %llu neg_tiles %llu narrow_hits %llu aimed %llu\n", T.pairs,
             T.pop, T.tiles, T.full, T.neg, T.narrow_hits, T.aimed);
    }
    return T.viol ? 1 : 0;
  }
  const double asp = 16.0 / 9.0;
  const Cam cams[4] = {
      cam_init({13, 2, 3}, {0, 0, 0}, {0, 1, 0}, 20.0, asp, 0.1, 10.0, 0.0, 1.0),   // the cover camera
      cam_init({13, 2, 3}, {0, 0, 0}, {0, 1, 0}, 20.0, asp, 2.0, 10.0, 0.0, 1.0),   // aperture 2.0
      cam_init({13, 2, 3}, {0, 0, 0}, {0, 1, 0}, 20.0, asp, 0.1, 1.0, 0.0, 1.0),    // focus distance 1
      cam_init({13, 0.3, 3}, {-13, 0.3, -3}, {0, 1, 0}, 40.0, asp, 0.1, 10.0, 0.0, 1.0)};  // along the ground plane
  const uint32_t frames[2][2] = {{96, 54}, {9, 9}}, splits[2][2] = {{0, 1}, {1, 3}};
  Totals T;
  for (const Cam& c : cams)
    for (const auto& fr : frames)
      for (const auto& sp : splits)
        run_frame(S, c, fr[0], fr[1], sp[0], sp[1], (fr[1] - sp[0] + sp[1] - 1) / sp[1], true, false, T);
  printf("rays %llu hits %llu violations %llu\n", T.rays, T.hits, T.viol);
  if (argc > 2 && std::strcmp(argv[2], "popcount") == 0) {
    Totals P;
    run_frame(S, cams[0], 1200, 675, 0, 1, 675, false, false, P);
    printf("mean_popcount %.3f of %llu narrow spheres over %llu tiles\n", (double)P.pop / (double)P.tiles,
           P.pairs / P.tiles, P.tiles);
  }
  return T.viol ? 1 : 0;
}
