// Precision mode of the emulation harnesses (emu_main.cc, local_emu_main.cc): the error of a product against double in units of
// 2^-24 of sum|a b| (tests/test_split_arithmetic_gpu.py's measure), on N(0,1) data and on data whose terms cancel in pairs.
#pragma once
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

namespace prec {
// The bounds, calibrated in emulation.  Measured on the kernels as they are: N(0,1) 0.7-3.6 units, cancelling pairs 0.01-1.04.  A
// build whose split_mac skips the m*m product: 6.3-38 (N(0,1)) and 3.7-42 (cancelling); filter planes with a zero l plane: 25-74
// (N(0,1); the l terms of a pair cancel with it, so only the N(0,1) family sees that mutant).  The 1e-4 parity cases pass both mutants.
constexpr double kNormal = 8.0, kCancel = 2.0;

// View a as [outer][len][inner] and pair slices 2i, 2i+1 along len: repeat (odd = even * (1 + 2^-12 r)) or negate (odd = -even; an odd
// last slice is zeroed, so every term has its partner).  With a repeated on one operand and negated on the other along the axis a
// product reduces over, every pair of terms cancels to ~2^-12 of its magnitude.
inline void pair(float* a, size_t outer, size_t len, size_t inner, bool negate, std::mt19937& rng) {
  std::normal_distribution<float> nd;
  for (size_t o = 0; o < outer; ++o)
    for (size_t l = 0; l + 1 < len; l += 2)
      for (size_t i = 0; i < inner; ++i) {
        float* e = a + (o * len + l) * inner + i;
        e[inner] = negate ? -e[0] : e[0] * (1.f + std::ldexp(nd(rng), -12));
      }
  if (negate && len % 2)
    for (size_t o = 0; o < outer; ++o)
      for (size_t i = 0; i < inner; ++i) a[(o * len + len - 1) * inner + i] = 0.f;
}

// max |out - ref| / mag over the outputs with mag > 0, in units of 2^-24
inline double err(const float* out, const std::vector<double>& ref, const std::vector<double>& mag) {
  double e = 0;
  for (size_t i = 0; i < ref.size(); ++i)
    if (mag[i] > 0) {
      const double v = std::fabs((double)out[i] - ref[i]) / mag[i];
      e = std::isfinite(v) ? std::max(e, v) : 1e300;
    }
  return e * 16777216.0;
}

inline bool verdict(const char* what, const char* family, double e) {
  const bool ok = e <= (family[0] == 'c' ? kCancel : kNormal);
  std::printf("%s prec %-13s %s err=%.4f x 2^-24 of sum|ab|\n", ok ? "PASS" : "FAIL", family, what, e);
  std::fflush(stdout);
  return ok;
}
}  // namespace prec
