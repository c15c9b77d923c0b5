// beam_bound_check — the tile-beam bound (csrc/rtw_beam.hpp) is conservative:
// for every 8x8 tile of a frame, rays made by Camera.getRay's formulas
// (main.zig:91-100, :390-391) at the extremes of the tile's parameters — jitter
// 0 and 1 - ulp, lens points on the unit circle and at 0, both shutter ends —
// and at seeded random values are solved exactly (f64, Sphere.hit /
// MovingSphere.hit, hittable.zig:95-131, :165-201) against every sphere; a
// sphere with a root >= tmin must be in the tile's mask.
//   beam_bound_check <scene.txt> [popcount]
// scene.txt: n, then per sphere "c0.xyz c1.xyz radius t0 t1 moving".
// `popcount`: also print the mean mask popcount of the narrow spheres over the
// 1200x675 frame's tiles with the cover camera.
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
};

// One frame: every tile's mask; with `rays`, the exact solves against it.
void run_frame(const std::vector<Sph>& S, const Cam& c, uint32_t W, uint32_t H, uint32_t rb, uint32_t rs, bool rays,
               Totals& T) {
  const uint32_t rc = (H - rb + rs - 1) / rs;
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
        if (std::fabs(S[i].r) < 100.0) T.pop += mask[i] ? 1 : 0;
      }
      T.tiles++;
      if (!rays) continue;
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
      for (const auto& sp : splits) run_frame(S, c, fr[0], fr[1], sp[0], sp[1], true, T);
  printf("rays %llu hits %llu violations %llu\n", T.rays, T.hits, T.viol);
  if (argc > 2 && std::strcmp(argv[2], "popcount") == 0) {
    Totals P;
    run_frame(S, cams[0], 1200, 675, 0, 1, false, P);
    int narrow = 0;
    for (const auto& s : S) narrow += std::fabs(s.r) < 100.0;
    printf("mean_popcount %.3f of %d narrow spheres over %llu tiles\n", (double)P.pop / (double)P.tiles, narrow, P.tiles);
  }
  return T.viol ? 1 : 0;
}
