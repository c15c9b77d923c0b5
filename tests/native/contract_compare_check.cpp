// Teeth of tests/native/contract_compare.hpp, the comparator of
// gpu_contract_check: arrays in which exactly one value per family is wrong —
// one ulp off, the wrong sign of zero, a NaN against a number, a number
// against a NaN, one state bit — among values that must pass (equal numbers,
// NaNs of different payloads, equal zeros, infinities).  Prints the families
// as gpu_contract_check does; tests/test_gpu_contract.py (CPU part) checks
// that exactly the planted indices are reported.
#include <cmath>
#include <limits>
#include <vector>

#include "contract_compare.hpp"

template <typename T>
static T from_bits(typename cc::BitsOf<T>::type u) {
  T v;
  std::memcpy(&v, &u, sizeof(v));
  return v;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  const double nan1 = from_bits<double>(0x7FF8000000000000ull), nan2 = from_bits<double>(0xFFF0000000000001ull);
  const std::vector<double> want = {1.0, -0.0, 0.0, inf, nan1, 0x1p-1074, 3.141592653589793, -2.5, nan2, 0.0};
  int bad = 0;
  {
    std::vector<double> got = want;
    got[4] = nan2, got[8] = nan1;  // two NaNs are equal whatever their payloads
    got[6] = std::nextafter(got[6], 4.0);  // planted: index 6
    cc::Family f("one_ulp");
    f.check_array(got.data(), want.data(), got.size());
    f.print();
    bad += f.mismatches != 0;
  }
  {
    std::vector<double> got = want;
    got[1] = 0.0;  // planted: index 1, +0 for -0
    cc::Family f("zero_sign");
    f.check_array(got.data(), want.data(), got.size());
    f.print();
    bad += f.mismatches != 0;
  }
  {
    std::vector<float> w = {1.0f, std::numeric_limits<float>::quiet_NaN(), 2.0f, -0.0f}, got = w;
    got[2] = std::numeric_limits<float>::quiet_NaN();  // planted: index 2, NaN for a number
    got[1] = -std::numeric_limits<float>::quiet_NaN();
    cc::Family f("nan_for_number");
    f.check_array(got.data(), w.data(), got.size());
    f.print();
    bad += f.mismatches != 0;
  }
  {
    std::vector<double> got = want;
    got[4] = 1.0;  // planted: index 4, a number for a NaN
    cc::Family f("number_for_nan");
    f.check_array(got.data(), want.data(), got.size());
    f.print();
    bad += f.mismatches != 0;
  }
  {
    std::vector<uint64_t> w = {0, 1, 0x9E3779B97F4A7C15ull, ~0ull}, got = w;
    got[3] ^= 1ull << 63;  // planted: index 3
    cc::Family f("state_bit");
    f.check_array(got.data(), w.data(), got.size());
    f.print();
    bad += f.mismatches != 0;
  }
  {
    std::vector<int32_t> w = {-1, 0, 1}, got = w;
    cc::Family f("all_equal");
    f.check_array(got.data(), w.data(), got.size());
    f.print();
    bad += f.mismatches != 0;
  }
  std::printf("ulp_distance %llu %llu %llu %llu\n", (unsigned long long)cc::ulp_distance(1.0, std::nextafter(1.0, 2.0)),
              (unsigned long long)cc::ulp_distance(-0.0, 0.0), (unsigned long long)cc::ulp_distance(nan1, nan2),
              (unsigned long long)(cc::ulp_distance(nan1, 1.0) == UINT64_MAX));
  return bad == 5 ? 0 : 1;
}
