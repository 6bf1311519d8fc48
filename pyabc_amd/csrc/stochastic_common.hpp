// Device helpers shared by the stochastic-acceptance units (stochastic.hip,
// stochastic_full.hip): one definition of the decision and of the Philox
// uniform, so every kernel decides an evaluation the same way.
#pragma once

#include "common.hpp"
#include "philox.hpp"

namespace abc {

constexpr int kPwDepth = 5;          // S <= 128 * 2^5 = 4096
constexpr int kMaxStats = 128 << kPwDepth;

__device__ inline double ulp_of(double x) {
  const double a = fabs(x);
  return nextafter(a, INFINITY) - a;
}

// acceptance of one evaluation: probability, decision, weight, guard flag
__device__ inline void stochastic_decide(double pd, double pdf_norm,
                                         double inv_temp, int log_scale,
                                         int apply_iw, double u,
                                         uint8_t& accept, double& weight,
                                         uint8_t& guard) {
#pragma clang fp contract(off)
  const double acc = log_scale ? exp((pd - pdf_norm) * inv_temp)
                               : pow(pd / pdf_norm, inv_temp);
  accept = acc >= u ? 1 : 0;
  weight = acc == 0.0 ? 0.0 : (apply_iw ? acc / fmin(1.0, acc) : 1.0);
  guard = (acc < 1.0 && fabs(acc - u) <= 4.0 * ulp_of(fmax(acc, u))) ? 1 : 0;
}

__device__ inline double philox_u01(uint64_t seed, uint64_t stream, uint64_t i) {
  const u32x4 b = philox_block(seed, stream, i >> 1);
  return (i & 1) ? u53(b.z, b.w) : u53(b.x, b.y);
}

}  // namespace abc
