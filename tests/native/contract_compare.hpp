// Bit-for-bit comparator of tests/native/gpu_contract_check.hip (plain C++: the
// CPU suite feeds it known-wrong arrays, tests/native/contract_compare_check.cpp).
// Two values are equal when their bit patterns are, or when both are NaN; +0
// and -0 differ, a NaN and a number differ.  One Family per input family:
// it counts cases and mismatches, keeps the first few mismatching indices and
// prints "family <name> cases N mismatches M" followed by those cases in hex.
#pragma once
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace cc {

template <typename T>
struct BitsOf;
template <>
struct BitsOf<double> { using type = uint64_t; };
template <>
struct BitsOf<float> { using type = uint32_t; };
template <>
struct BitsOf<uint64_t> { using type = uint64_t; };
template <>
struct BitsOf<uint32_t> { using type = uint32_t; };
template <>
struct BitsOf<int32_t> { using type = uint32_t; };

template <typename T>
inline uint64_t bits(T v) {
  typename BitsOf<T>::type u;
  static_assert(sizeof(u) == sizeof(v), "size");
  std::memcpy(&u, &v, sizeof(v));
  return (uint64_t)u;
}
inline bool is_nan(double v) { return v != v; }
inline bool is_nan(float v) { return v != v; }
inline bool is_nan(uint64_t) { return false; }
inline bool is_nan(uint32_t) { return false; }
inline bool is_nan(int32_t) { return false; }

template <typename T>
inline bool same(T got, T want) {
  return bits(got) == bits(want) || (is_nan(got) && is_nan(want));
}

// |a - b| in units in the last place (monotone bit-pattern distance); 0 for two NaNs,
// UINT64_MAX for a NaN against a number
inline uint64_t ulp_distance(double a, double b) {
  if (a != a || b != b) return (a != a && b != b) ? 0 : UINT64_MAX;
  auto key = [](double x) {
    const uint64_t u = bits(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);  // order-preserving (-0 just below +0)
  };
  const uint64_t ka = key(a), kb = key(b);
  return ka > kb ? ka - kb : kb - ka;
}

struct Family {
  std::string name;
  uint64_t cases = 0, mismatches = 0;
  struct Miss {
    uint64_t index, in0, in1, got, want;
  };
  std::vector<Miss> first;
  static constexpr size_t kKeep = 8;

  explicit Family(const char* n) : name(n) {}
  // in0 / in1: the case's inputs as bit patterns, for the report only
  template <typename T>
  void check(uint64_t index, uint64_t in0, uint64_t in1, T got, T want) {
    ++cases;
    if (same(got, want)) return;
    ++mismatches;
    if (first.size() < kKeep) first.push_back({index, in0, in1, bits(got), bits(want)});
  }
  // got[i] against want[i], the index as the only input
  template <typename T>
  void check_array(const T* got, const T* want, size_t n) {
    for (size_t i = 0; i < n; ++i) check(i, i, 0, got[i], want[i]);
  }
  void print(FILE* f = stdout) const {
    std::fprintf(f, "family %s cases %" PRIu64 " mismatches %" PRIu64 "\n", name.c_str(), cases, mismatches);
    for (const Miss& m : first)
      std::fprintf(f, "  mismatch %s index %" PRIu64 " in 0x%016" PRIx64 " 0x%016" PRIx64 " got 0x%016" PRIx64 " want 0x%016" PRIx64 "\n",
                   name.c_str(), m.index, m.in0, m.in1, m.got, m.want);
  }
};

}  // namespace cc
