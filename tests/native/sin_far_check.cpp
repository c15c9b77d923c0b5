// sin_far_check — rtwl::sin_far (rtw_libm.hpp), the device's sin for
// 2^20 * pi/2 <= |x| < 2^32, built for the host and held against a file of
// correctly rounded values: pairs of little-endian doubles (x, sin x rounded to
// nearest, computed with 400-bit arithmetic).  The inputs: the range a scale-4
// noise texture reaches with |p| <= 1e6, every binade up to 2^32, both signs,
// the doubles next to 2,000 multiples of pi/2 (the reductions that cancel), and
// the range's two ends.  The platform's own sin is counted beside it and
// asserts nothing.
//
//   sin_far_check FILE  ->  "cases N mismatches M platform_differs K", exit 1 if M != 0
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rtw_libm.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<double> v;
  double pair[2];
  while (std::fread(pair, sizeof(double), 2, f) == 2) v.push_back(pair[0]), v.push_back(pair[1]);
  std::fclose(f);
  unsigned long long bad = 0, platform = 0;
  for (size_t i = 0; i < v.size(); i += 2) {
    const double x = v[i], want = v[i + 1], got = rtwl::sin_far(x);
    if (!(std::fabs(x) >= 1647099.0 && std::fabs(x) < 0x1p32)) return 2;
    if (rtwl::bits(got) != rtwl::bits(want)) {
      if (bad++ < 5) std::printf("x %a got %a want %a\n", x, got, want);
    }
    if (rtwl::bits(std::sin(x)) != rtwl::bits(want)) ++platform;
  }
  std::printf("cases %zu mismatches %llu platform_differs %llu\n", v.size() / 2, bad, platform);
  return bad != 0;
}
