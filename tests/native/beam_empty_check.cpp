// beam_empty_check — the megakernel's "proven empty" rule for a tile (rtw_trace.hip take_units,
// TraceArgs::empty_on): csrc/rtw_beam.hpp's bound answers "cannot be hit" for EVERY sphere of the
// scene, wide ones included.  For every tile the rule proves empty, rays made by Camera.getRay's
// formulas (main.zig:91-100, :390-391) are solved exactly in f64 against every sphere (Sphere.hit /
// MovingSphere.hit, hittable.zig:95-131, :165-201): the tile's corners and edge midpoints (jitter 0
// and 1 - ulp), from 8 lens-rim points and the lens centre, at both shutter ends, plus 64 seeded
// random rays per tile.  A root >= 0 of any sphere is a violation.
//   beam_empty_check <scene.txt> <cases.txt> [list]
// scene.txt, cases.txt: the formats of beam_bound_check.cpp (tests/helpers.py write_beam_scene,
// write_beam_cases).  Per case prints "case i tiles T empty E rays R violations V"; with `list`, a
// line "empty i: t0 t1 ..." of the proven tiles' indices (ty * tiles_x + tx) as well.  Exit status 1
// when any case has a violation.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rtw_beam.hpp"

namespace {

struct Sph {
  double c0[3], c1[3], r, t0, t1;
  int moving;
};
struct Cam {
  double o[3], hor[3], ver[3], llc[3], u[3], v[3], lens, time0, time1;
};

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
double rnd() {  // xorshift64*, [0, 1)
  g_rng ^= g_rng >> 12, g_rng ^= g_rng << 25, g_rng ^= g_rng >> 27;
  return (double)((g_rng * 0x2545F4914F6CDD1Dull) >> 11) * 0x1p-53;
}

// Any root >= 0 of the ray o + l d (its larger root is: root2 >= root1).
bool root_ge0(const Sph& s, const double o[3], const double d[3], double time) {
  double c[3], oc[3], a = 0, hb = 0, cc = 0;
  const double fr = s.moving ? (time - s.t0) / (s.t1 - s.t0) : 0.0;
  for (int k = 0; k < 3; ++k) {
    c[k] = s.c0[k] + (s.moving ? (s.c1[k] - s.c0[k]) * fr : 0.0);
    oc[k] = o[k] - c[k];
    a += d[k] * d[k], hb += oc[k] * d[k], cc += oc[k] * oc[k];
  }
  cc -= s.r * s.r;
  const double disc = hb * hb - a * cc;
  if (disc < 0.0) return false;
  return !((-hb + std::sqrt(disc)) / a < 0.0);
}

// Camera.getRay with pixel parameters (s, t), lens point (dx, dy) of the unit disk.
bool ray_hits(const std::vector<Sph>& S, const Cam& c, double s, double t, double dx, double dy, double time) {
  double o[3], d[3];
  for (int k = 0; k < 3; ++k) {
    const double off = c.u[k] * (c.lens * dx) + c.v[k] * (c.lens * dy);
    o[k] = c.o[k] + off;
    d[k] = c.llc[k] + s * c.hor[k] + t * c.ver[k] - c.o[k] - off;
  }
  for (const Sph& sp : S)
    if (root_ge0(sp, o, d, time)) return true;
  return false;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const bool list = argc > 3 && std::strcmp(argv[3], "list") == 0;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n = 0;
  if (std::fscanf(f, "%d", &n) != 1) return 2;
  std::vector<Sph> S(n);
  for (Sph& s : S)
    if (std::fscanf(f, "%lf %lf %lf %lf %lf %lf %lf %lf %lf %d", &s.c0[0], &s.c0[1], &s.c0[2], &s.c1[0], &s.c1[1], &s.c1[2],
                    &s.r, &s.t0, &s.t1, &s.moving) != 10)
      return 2;
  std::fclose(f);
  f = std::fopen(argv[2], "r");
  if (!f) return 2;
  int nc = 0;
  if (std::fscanf(f, "%d", &nc) != 1) return 2;
  const double one_m = std::nextafter(1.0, 0.0);
  unsigned long long viol_all = 0;
  for (int ci = 0; ci < nc; ++ci) {
    Cam c;
    uint32_t W, H, rb, rs, rc;
    double* v[6] = {c.o, c.hor, c.ver, c.llc, c.u, c.v};
    for (auto* p : v)
      if (std::fscanf(f, "%lf %lf %lf", p, p + 1, p + 2) != 3) return 2;
    if (std::fscanf(f, "%lf %lf %lf %u %u %u %u %u", &c.lens, &c.time0, &c.time1, &W, &H, &rb, &rs, &rc) != 8) return 2;
    unsigned long long tiles = 0, rays = 0, viol = 0;
    std::vector<uint32_t> empty;
    const uint32_t tiles_x = (W + 7) / 8;
    for (uint32_t ty = 0; ty * 8 < rc; ++ty)
      for (uint32_t tx = 0; tx < tiles_x; ++tx, ++tiles) {
        const uint32_t px0 = tx * 8, px1 = std::min(px0 + 7, W - 1), ly0 = ty * 8, ly1 = std::min(ly0 + 7, rc - 1);
        const uint32_t y0 = rb + ly0 * rs, y1 = rb + ly1 * rs;
        const rtwb::Beam b = rtwb::tile_beam(c.o, c.llc, c.hor, c.ver, c.u, c.v, c.lens, W, H, px0, px1, y0, y1);
        bool may = false;
        for (const Sph& s : S) {
          const double dc[3] = {s.c1[0] - s.c0[0], s.c1[1] - s.c0[1], s.c1[2] - s.c0[2]};
          may = may || rtwb::beam_may_hit(b, s.c0, dc, s.r, s.moving != 0, s.t0, s.t1, c.time0, c.time1);
        }
        if (may) continue;
        empty.push_back(ty * tiles_x + tx);
        // u of column px with jitter j: (px + j) / (W - 1); v of image row y: (H - 1 - y + j) / (H - 1)
        const double w1 = (double)W - 1.0, h1 = (double)H - 1.0;
        const double s_lo = (double)px0 / w1, s_hi = ((double)px1 + one_m) / w1;
        const double t_lo = ((double)(H - 1 - y1)) / h1, t_hi = ((double)(H - 1 - y0) + one_m) / h1;
        const double ss[3] = {s_lo, 0.5 * (s_lo + s_hi), s_hi}, ts[3] = {t_lo, 0.5 * (t_lo + t_hi), t_hi};
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) {
            if (i == 1 && j == 1) continue;  // corners and edge midpoints
            for (int li = 0; li < 9; ++li) {
              const double ang = li * (M_PI / 4.0), dx = li < 8 ? std::cos(ang) : 0.0, dy = li < 8 ? std::sin(ang) : 0.0;
              for (double tm : {c.time0, c.time1}) rays++, viol += ray_hits(S, c, ss[i], ts[j], dx, dy, tm) ? 1 : 0;
            }
          }
        for (int k = 0; k < 64; ++k) {
          const uint32_t px = px0 + (uint32_t)(rnd() * (px1 - px0 + 1)), ly = ly0 + (uint32_t)(rnd() * (ly1 - ly0 + 1));
          const double s = ((double)px + rnd()) / w1, t = ((double)(H - 1 - (rb + ly * rs)) + rnd()) / h1;
          double dx, dy;
          do dx = 2.0 * rnd() - 1.0, dy = 2.0 * rnd() - 1.0;
          while (dx * dx + dy * dy >= 1.0);
          rays++, viol += ray_hits(S, c, s, t, dx, dy, c.time0 + (c.time1 - c.time0) * rnd()) ? 1 : 0;
        }
      }
    std::printf("case %d tiles %llu empty %zu rays %llu violations %llu\n", ci, tiles, empty.size(), rays, viol);
    if (list) {
      std::printf("empty %d:", ci);
      for (uint32_t t : empty) std::printf(" %u", t);
      std::printf("\n");
    }
    viol_all += viol;
  }
  std::fclose(f);
  return viol_all ? 1 : 0;
}
