// tri_exact_probe — csrc/rtw_tri.hpp evaluated on (triangle, ray) pairs read from a
// file, for tests/test_tri_exact_host.py to compare with the rational reference
// (tests/tri_exact.py).  Plain C++, -ffp-contract=off, no HIP.
//   input   "T v0x .. v2z"            a triangle (nine hexfloats); numbered in order
//           "R tri ox oy oz dx dy dz"  an object-space ray against triangle `tri`
//   output  one line per ray:
//           "ok inside hit t u v front nx ny nz"
//   ok: derive's verdict; inside: inside_ray; hit: root with t_min = -inf; t: the
//   plane root (nan when the ray lies in the plane); u, v: bary; front: n . d < 0;
//   n: the unit normal, facing the ray.  Doubles are printed with %a.
#include <cmath>
#include <cstdio>
#include <vector>

#include "rtw_tri.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<double> tris;
  char tag[4];
  while (std::fscanf(f, "%3s", tag) == 1) {
    if (tag[0] == 'T') {
      double a[9];
      for (int k = 0; k < 9; ++k)
        if (std::fscanf(f, "%la", &a[k]) != 1) return 3;
      tris.insert(tris.end(), a, a + 9);
    } else if (tag[0] == 'R') {
      unsigned long i;
      double r[6];
      if (std::fscanf(f, "%lu", &i) != 1 || 9 * (i + 1) > tris.size()) return 3;
      for (int k = 0; k < 6; ++k)
        if (std::fscanf(f, "%la", &r[k]) != 1) return 3;
      const double* a = &tris[9 * i];
      double n[3], h, t = NAN, tp = NAN, u, v;
      const bool ok = rtwtri::derive(a, n, h);
      const bool inside = rtwtri::inside_ray(a, r[0], r[1], r[2], r[3], r[4], r[5]);
      const bool hit = rtwtri::root(a, n[0], n[1], n[2], h, r[0], r[1], r[2], r[3], r[4], r[5], -INFINITY, t);
      (void)rtwtri::plane_t(n[0], n[1], n[2], h, r[0], r[1], r[2], r[3], r[4], r[5], tp);
      rtwtri::bary(a, r[0], r[1], r[2], r[3], r[4], r[5], u, v);
      const bool front = n[0] * r[3] + n[1] * r[4] + n[2] * r[5] < 0.0;
      const double s = front ? 1.0 : -1.0;
      std::printf("%d %d %d %a %a %a %d %a %a %a\n", (int)ok, (int)inside, (int)hit, hit ? t : tp, u, v, (int)front,
                  n[0] * s, n[1] * s, n[2] * s);
    } else {
      return 3;
    }
  }
  std::fclose(f);
  return 0;
}
