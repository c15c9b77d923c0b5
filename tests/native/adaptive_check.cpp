// Host check of the adaptive-sampling criterion (csrc/rtw_adaptive.hpp), the
// function the accumulator's kernels compile.  Reads a table of cases from the
// file named on the command line, one per line:
//   SY SY2 cnt chunk min_spp thr want_converged want_se2
// with the doubles as hexadecimal bit patterns (want_se2 ignored for m < 2),
// as tests/test_adaptive_cpu.py computed them in numpy f64, and compares case
// by case: the flag, and se2 bit for bit.  Exit status 0 when all agree.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "rtw_adaptive.hpp"

static double from_bits(uint64_t b) {
  double d;
  std::memcpy(&d, &b, 8);
  return d;
}
static uint64_t to_bits(double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  uint64_t sy, sy2, thr, want_se2;
  uint32_t cnt, chunk, min_spp, want;
  int n = 0, bad = 0;
  while (std::fscanf(f, "%" SCNx64 " %" SCNx64 " %u %u %u %" SCNx64 " %u %" SCNx64, &sy, &sy2, &cnt, &chunk, &min_spp,
                     &thr, &want, &want_se2) == 8) {
    const bool got = rtwa::pixel_converged(from_bits(sy), from_bits(sy2), cnt, chunk, min_spp, from_bits(thr));
    const uint32_t m = cnt / chunk;
    bool ok = got == (want != 0);
    uint64_t se2 = 0;
    if (m >= 2) {
      se2 = to_bits(rtwa::pixel_se2(from_bits(sy), from_bits(sy2), m, chunk));
      ok = ok && se2 == want_se2;
    }
    if (!ok) {
      ++bad;
      std::printf("case %d: converged %d want %u, se2 %016" PRIx64 " want %016" PRIx64 "\n", n, (int)got, want, se2,
                  want_se2);
    }
    ++n;
  }
  std::fclose(f);
  std::printf("adaptive_check: bad %d/%d\n", bad, n);
  return bad == 0 && n > 0 ? 0 : 1;
}
