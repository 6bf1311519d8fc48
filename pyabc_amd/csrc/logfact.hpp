// Log-factorial lf(m) = lgamma(m + 1) for the count-data kernels
// (stochastic_count.hip), host and device alike so the maths can be checked
// against a multiprecision reference on a CPU.
//
//   m <  kLfTable : a table entry, built by lf_table_entry from double-double
//                   logarithms and correctly rounded up to 1 ulp;
//   m >= kLfTable : lf_stirling, the Stirling series in 1 / (m + 1).
//
// Everything here is written with explicit fma and contraction off, so host
// and device agree bit for bit apart from the libm log inside lf_stirling.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define ABC_HD __host__ __device__
#else
#define ABC_HD
#endif

namespace abc {

constexpr int kLfTable = 4096;  // entries per table (power of two), 32 KiB

// ---- double-double: value = hi + lo, |lo| <= ulp(hi) / 2 -------------------
struct dd {
  double hi, lo;
};

ABC_HD inline dd two_sum(double a, double b) {
#pragma clang fp contract(off)
  const double s = a + b;
  const double bb = s - a;
  return dd{s, (a - (s - bb)) + (b - bb)};
}

ABC_HD inline dd two_prod(double a, double b) {
  const double p = a * b;
  return dd{p, fma(a, b, -p)};
}

ABC_HD inline dd dd_add(dd a, dd b) {
#pragma clang fp contract(off)
  const dd s = two_sum(a.hi, b.hi);
  return two_sum(s.hi, s.lo + (a.lo + b.lo));
}

// log(j) for an integer 1 <= j < 2^53 to ~1e-18 absolute:
//   j = 2^e f, f in [sqrt(1/2), sqrt(2)),  log f = 2 atanh(s), s = (f-1)/(f+1)
// s as a double-double quotient (f -+ 1 are exact), the series tail
// s^3 (1/3 + s^2/5 + ...) in plain fp64: |s| <= 0.172, so the tail is below
// 1.7e-3 and its rounding below 1e-18; 13 terms leave s^28 / 29 < 1e-22.
ABC_HD inline dd dd_log_int(double j) {
#pragma clang fp contract(off)
  int e;
  double f = frexp(j, &e);  // [0.5, 1)
  if (f < 0.70710678118654752) {
    f *= 2.0;
    e -= 1;
  }
  const double a = f - 1.0, b = f + 1.0;
  const double q1 = a / b;
  const double q2 = fma(-q1, b, a) / b;
  const double z = q1 * q1;
  double p = 1.0 / 27.0;
  p = fma(p, z, 1.0 / 25.0);
  p = fma(p, z, 1.0 / 23.0);
  p = fma(p, z, 1.0 / 21.0);
  p = fma(p, z, 1.0 / 19.0);
  p = fma(p, z, 1.0 / 17.0);
  p = fma(p, z, 1.0 / 15.0);
  p = fma(p, z, 1.0 / 13.0);
  p = fma(p, z, 1.0 / 11.0);
  p = fma(p, z, 1.0 / 9.0);
  p = fma(p, z, 1.0 / 7.0);
  p = fma(p, z, 1.0 / 5.0);
  p = fma(p, z, 1.0 / 3.0);
  const double tail = (q1 * z) * p;
  // fdlibm's split of log 2: the high part has 21 trailing zero bits, so
  // e * kLn2Hi is exact for |e| < 2^20
  constexpr double kLn2Hi = 6.93147180369123816490e-01;
  constexpr double kLn2Lo = 1.90821492927058770002e-10;
  const dd s = two_sum(e * kLn2Hi, 2.0 * q1);
  return two_sum(s.hi, s.lo + fma(static_cast<double>(e), kLn2Lo,
                                  2.0 * (q2 + tail)));
}

// lf(m) for 0 <= m < kLfTable as the double-double sum of log 2 .. log m,
// rounded once: each logarithm is good to 1e-18, so 4095 of them stay four
// orders of magnitude below half an ulp of any entry (the smallest nonzero
// entry is log 2, ulp 1.1e-16).
ABC_HD inline double lf_table_entry(int m) {
  dd s{0.0, 0.0};
  for (int j = 2; j <= m; ++j) s = dd_add(s, dd_log_int(static_cast<double>(j)));
  return s.hi;
}

// log(m) for 1 <= m < kLfTable, correctly rounded up to 1e-18; entry 0 is 0
// (the kernel decides log 0 by flag, never by arithmetic on -inf)
ABC_HD inline double log_table_entry(int m) {
  return m < 2 ? 0.0 : dd_log_int(static_cast<double>(m)).hi;
}

// lf(m) for an integer m >= kLfTable, x = m + 1:
//   lgamma(x) = (x - 1/2) log x - x + log(2 pi)/2 + 1/(12 x) - 1/(360 x^3) + R
// |R| < 1/(1260 x^5) < 7e-22 at x = 4097, i.e. 2^-85 of the value 29978.
// The small terms need 1/x to ~1e-8 only (they are below 2.1e-5 against an ulp
// of 3.6e-12): a float reciprocal and one Newton step.  The dominant part is
// one fma, fma(x - 1/2, log x, c - x): the product is not rounded, and c - x
// rounds at ulp(x) <= ulp(result) / 7.  Error: the log's e_L ulp are amplified
// by L / (L - 1) <= 1.137, so in units of 2^-53 of the result
//   2 * 1.137 * e_L + 0.15 + 1 = 3.43 for a 1-ulp log.
ABC_HD inline double lf_stirling(double m) {
#pragma clang fp contract(off)
  const double x = m + 1.0;
#if defined(__HIP_DEVICE_COMPILE__)
  double w = static_cast<double>(__builtin_amdgcn_rcpf(static_cast<float>(x)));
#else
  double w = static_cast<double>(1.0f / static_cast<float>(x));
#endif
  w = w * fma(-x, w, 2.0);
  constexpr double kHalfLog2Pi = 0.91893853320467274178;
  const double w2 = w * w;
  const double c = fma(w, fma(w2, -1.0 / 360.0, 1.0 / 12.0), kHalfLog2Pi);
  return fma(x - 0.5, log(x), c - x);
}

}  // namespace abc
