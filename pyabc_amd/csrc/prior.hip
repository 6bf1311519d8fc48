// Priors beyond the uniform box: the log density, density and support flag
// of a product of scipy.stats marginals (abc_prior_logpdf_f64) and its draws
// (abc_prior_rvs_f64), both driven by the host's marginal table
// (abc_prior_table, include/abc_hip.h; DESIGN.md, "Prior table").
//
// How the work is split and where the data lives:
//   * a block owns a tile of kPriorRows consecutive rows of theta [B][d]: a
//     contiguous run of rows * d doubles.  The density kernel copies the run
//     to LDS with coalesced loads (lane t takes elements t, t + 128, ...), the
//     draw kernel writes its results to LDS and copies the run out the same
//     way; in between ONE LANE OWNS ONE ROW and walks its d entries in LDS.
//     The LDS row stride is d | 1 doubles (odd: the 64 lanes of a wave, rows
//     apart, hit distinct bank pairs for every column);
//   * the part of the table a kernel reads is a kernel argument BY VALUE
//     (2944 / 1920 bytes of the 4 KiB argument segment).  The dimension index
//     k is the same for every lane, so each table read is a scalar load, the
//     coefficients sit in SGPRs, and the tests of the term mask and of the
//     family are scalar branches: a dimension costs the transcendentals its
//     family has and no others (none for uniform and norm, one log for gamma,
//     log and log1p for beta).  A per-element kernel (k = i % d per lane)
//     would index the table by a vector value, i.e. from scratch;
//   * a masked-off term is skipped, never multiplied by zero: 0 * log(z) is
//     NaN for z <= 0.
// The rejection loops of gamma and beta are bounded (ABC_PRIOR_GAMMA_TRIES
// tries, then NaN): lanes leave them one by one and nothing spins.
// No matrix instructions: a row is d <= 32 independent scalar transforms.
#include "common.hpp"
#include "philox.hpp"
#include "../../include/abc_hip.h"

namespace abc {

constexpr int kPriorRows = 128;  // rows of a tile = lanes of a block
constexpr int kD = ABC_PRIOR_MAX_DIM;

// the table's leading fields, loc .. mask: what the density reads
struct PriorDensity {
  double loc[kD], scale[kD], zlo[kD], zhi[kD], c[kD], a[kD], b[kD], e[kD], f[kD],
      g[kD], k[kD];
  int32_t mask[kD];
};
// what the draws read: loc .. zhi and the table's trailing fields p0 .. family
struct PriorDraw {
  double loc[kD], scale[kD], zlo[kD], zhi[kD], p0[kD], p1[kD], p2[kD];
  int32_t family[kD];
};
static_assert(sizeof(abc_prior_table) == 3840, "abc_prior_table layout (abc_hip.h)");
static_assert(sizeof(PriorDensity) == offsetof(abc_prior_table, p0), "density prefix");
static_assert(sizeof(PriorDraw) == 4 * kD * sizeof(double) + sizeof(abc_prior_table) -
                                       offsetof(abc_prior_table, p0),
              "draw fields");

__global__ __launch_bounds__(kPriorRows) void prior_logpdf_kernel(
    const PriorDensity T, const double* __restrict__ theta, int d, int64_t B,
    double* __restrict__ logp, double* __restrict__ pd, uint8_t* __restrict__ sup) {
  extern __shared__ double tile[];  // [kPriorRows][d | 1]
  const int ld = d | 1;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kPriorRows;
  const int rows = static_cast<int>(B - r0 < kPriorRows ? B - r0 : kPriorRows);
  const double* src = theta + r0 * d;
  const unsigned n = static_cast<unsigned>(rows * d), ud = static_cast<unsigned>(d);
  for (unsigned i = threadIdx.x; i < n; i += kPriorRows) {
    const unsigned r = i / ud;
    tile[r * ld + (i - r * ud)] = src[i];
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) >= rows) return;
  const double* x = tile + threadIdx.x * ld;
  double lp = 0.0;
  bool ok = true;
  for (int k = 0; k < d; ++k) {
    const int m = T.mask[k];
    const double z = (x[k] - T.loc[k]) / T.scale[k];
    const bool lo = (m & ABC_PRIOR_LO_CLOSED) ? z >= T.zlo[k] : z > T.zlo[k];
    const bool hi = (m & ABC_PRIOR_HI_CLOSED) ? z <= T.zhi[k] : z < T.zhi[k];
    // a NaN fails both compares; every density is 0 at an infinite z
    ok = ok && lo && hi && fabs(z) < INFINITY;
    double t = T.c[k];
    if (m & (ABC_PRIOR_TERM_LOGZ | ABC_PRIOR_TERM_LOGSQ)) {
      const double l = log(z);
      if (m & ABC_PRIOR_TERM_LOGZ) t = fma(T.a[k], l, t);
      if (m & ABC_PRIOR_TERM_LOGSQ) t = fma(-T.k[k], l * l, t);
    }
    if (m & ABC_PRIOR_TERM_LOG1M) t = fma(T.b[k], log1p(-z), t);
    if (m & ABC_PRIOR_TERM_LIN) t = fma(-T.e[k], z, t);
    if (m & ABC_PRIOR_TERM_SQ) t = fma(-T.f[k], z * z, t);
    if (m & ABC_PRIOR_TERM_ABS) t = fma(-T.g[k], fabs(z), t);
    lp += t;
  }
  // outside the support the sum may hold anything (log of a negative z)
  lp = ok ? lp : -INFINITY;
  const double p = exp(lp);
  const int64_t row = r0 + threadIdx.x;
  if (logp) logp[row] = lp;
  if (pd) pd[row] = p;
  if (sup) sup[row] = ok && p > 0.0 ? 1 : 0;
}

// one gamma(shape) variate (Marsaglia, Tsang 2000): x ~ N(0, 1) by inversion
// of words 0-1 of block base + t, v = (1 + c x)^3, accepted when
// log U < x^2 / 2 + d - d v + d log v with U of words 2-3; shape < 1 draws
// gamma(shape + 1) and multiplies by U'^(1 / shape), U' of block base + tries.
// x = -inf (a zero uniform) fails v > 0; U = 0 accepts, as log 0 = -inf.
// Not inlined and not unrolled: ONE copy of the loop serves gamma and both
// variates of beta.
__device__ __noinline__ double gamma_variate(double shape, uint64_t seed,
                                             uint64_t stream, uint64_t base) {
  const bool boost = shape < 1.0;
  const double dd = (boost ? shape + 1.0 : shape) - 1.0 / 3.0;
  const double cc = 1.0 / sqrt(9.0 * dd);
  double out = NAN;
  bool done = false;
#pragma unroll 1
  for (int t = 0; t < ABC_PRIOR_GAMMA_TRIES && !done; ++t) {
    const u32x4 blk = philox_block(seed, stream, base + static_cast<uint64_t>(t));
    const double x = normcdfinv(u53(blk.x, blk.y));
    double v = fma(cc, x, 1.0);
    if (v > 0.0) {
      v = v * v * v;
      const double lu = log(u53(blk.z, blk.w));
      if (lu < fma(0.5 * x, x, dd) - dd * v + dd * log(v)) {
        out = dd * v;
        done = true;
      }
    }
  }
  if (boost) {
    const u32x4 blk = philox_block(seed, stream, base + ABC_PRIOR_GAMMA_TRIES);
    out *= exp(log(fmax(u53(blk.x, blk.y), 0x1p-54)) / shape);
  }
  return out;
}

__global__ __launch_bounds__(kPriorRows) void prior_rvs_kernel(
    const PriorDraw T, int d, uint64_t seed, uint64_t sid, uint64_t offset, int64_t B,
    double* __restrict__ theta) {
  extern __shared__ double tile[];  // [kPriorRows][d | 1]
  const int ld = d | 1;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kPriorRows;
  const int rows = static_cast<int>(B - r0 < kPriorRows ? B - r0 : kPriorRows);
  if (static_cast<int>(threadIdx.x) < rows) {
    double* x = tile + threadIdx.x * ld;
    const uint64_t i0 =
        (offset + static_cast<uint64_t>(r0 + threadIdx.x)) * static_cast<uint64_t>(d);
#pragma unroll 1
    for (int k = 0; k < d; ++k) {
      const uint64_t i = i0 + static_cast<uint64_t>(k);
      const u32x4 ub = philox_block(seed, sid, i >> 1);
      const double u0 = (i & 1) ? u53(ub.z, ub.w) : u53(ub.x, ub.y);
      const int fam = T.family[k];
      // uniform takes u itself (abc_prior_uniform_f64's fma, bit for bit)
      const double u = fam == ABC_PRIOR_UNIFORM ? u0 : fmax(u0, 0x1p-54);
      double z = u;
      if (fam == ABC_PRIOR_NORM || fam == ABC_PRIOR_LOGNORM ||
          fam == ABC_PRIOR_TRUNCNORM) {
        // one inverse normal cdf for the three: of u, or for truncnorm of
        // the target cdf v while v <= 1/2 and else of the target upper tail
        // w (negated): either is a sum of positive masses, no cancellation
        double q = u;
        bool upper = false;
        if (fam == ABC_PRIOR_TRUNCNORM) {
          const double v = fma(u, T.p2[k], T.p0[k]);
          const double w = fma(1.0 - u, T.p2[k], T.p1[k]);
          upper = v > 0.5;
          q = upper ? w : v;
        }
        z = normcdfinv(q);
        z = upper ? -z : z;
        if (fam == ABC_PRIOR_LOGNORM) z = exp(T.p0[k] * z);
        // rounding of the masses can leave the draw an ulp outside
        if (fam == ABC_PRIOR_TRUNCNORM) z = fmin(fmax(z, T.zlo[k]), T.zhi[k]);
      } else if (fam == ABC_PRIOR_EXPON) {
        z = -log1p(-u);
      } else if (fam == ABC_PRIOR_LAPLACE) {
        z = u > 0.5 ? -log(2.0 * (1.0 - u)) : log(2.0 * u);
      } else if (fam == ABC_PRIOR_LOGUNIFORM) {
        z = exp(fma(u, T.p1[k], T.p0[k]));
      } else if (fam == ABC_PRIOR_GAMMA || fam == ABC_PRIOR_BETA) {
        const uint64_t base = i * ABC_PRIOR_DRAW_BLOCKS;
        z = gamma_variate(T.p0[k], seed, sid + 1, base);
        if (fam == ABC_PRIOR_BETA)
          z = z / (z + gamma_variate(T.p1[k], seed, sid + 1,
                                     base + ABC_PRIOR_DRAW_BLOCKS / 2));
      }
      x[k] = fma(T.scale[k], z, T.loc[k]);
    }
  }
  __syncthreads();
  double* dst = theta + r0 * d;
  const unsigned n = static_cast<unsigned>(rows * d), ud = static_cast<unsigned>(d);
  for (unsigned i = threadIdx.x; i < n; i += kPriorRows) {
    const unsigned r = i / ud;
    dst[i] = tile[r * ld + (i - r * ud)];
  }
}

static int check_table(const abc_prior_table* T, int d, const char* who) {
  ABC_REQUIRE(T, "%s: null table", who);
  ABC_REQUIRE(d >= 1 && d <= kD, "%s: 1 <= d <= 32", who);
  for (int k = 0; k < d; ++k) {
    ABC_REQUIRE(T->family[k] >= ABC_PRIOR_UNIFORM && T->family[k] <= ABC_PRIOR_BETA,
                "%s: family of marginal %d", who, k);
    ABC_REQUIRE(T->scale[k] > 0.0 && std::isfinite(T->scale[k]) &&
                    std::isfinite(T->loc[k]),
                "%s: loc / scale of marginal %d", who, k);
  }
  return kOk;
}

}  // namespace abc

using namespace abc;

extern "C" {

int abc_prior_logpdf_f64(const double* theta, const abc_prior_table* table, int d,
                         int64_t B, double* logp, double* pd, uint8_t* in_support,
                         hipStream_t st) {
  if (const int rc = check_table(table, d, "prior_logpdf")) return rc;
  ABC_REQUIRE(B >= 0, "prior_logpdf: B < 0");
  if (B == 0) return kOk;
  ABC_REQUIRE(theta, "prior_logpdf: null theta");
  PriorDensity T;
  memcpy(&T, table, sizeof(T));
  const size_t lds = static_cast<size_t>(kPriorRows) * (d | 1) * sizeof(double);
  hipLaunchKernelGGL(prior_logpdf_kernel,
                     dim3(static_cast<unsigned>(ceil_div(B, kPriorRows))),
                     dim3(kPriorRows), lds, st, T, theta, d, B, logp, pd, in_support);
  ABC_LAUNCH_CHECK("prior_logpdf_kernel");
  return kOk;
}

int abc_prior_rvs_f64(const abc_prior_table* table, int d, uint64_t seed,
                      uint64_t sid, uint64_t offset, int64_t B, double* theta,
                      hipStream_t st) {
  if (const int rc = check_table(table, d, "prior_rvs")) return rc;
  ABC_REQUIRE(B >= 0, "prior_rvs: B < 0");
  if (B == 0) return kOk;
  ABC_REQUIRE(theta, "prior_rvs: null theta");
  for (int k = 0; k < d; ++k) {
    const int fam = table->family[k];
    if (fam == ABC_PRIOR_GAMMA || fam == ABC_PRIOR_BETA)
      ABC_REQUIRE(table->p0[k] > 0.0 && std::isfinite(table->p0[k]) &&
                      (fam == ABC_PRIOR_GAMMA ||
                       (table->p1[k] > 0.0 && std::isfinite(table->p1[k]))),
                  "prior_rvs: shape of marginal %d", k);
  }
  PriorDraw T;
  memcpy(T.loc, table->loc, 4 * kD * sizeof(double));  // loc, scale, zlo, zhi
  memcpy(T.p0, table->p0, sizeof(abc_prior_table) - offsetof(abc_prior_table, p0));
  const size_t lds = static_cast<size_t>(kPriorRows) * (d | 1) * sizeof(double);
  hipLaunchKernelGGL(prior_rvs_kernel,
                     dim3(static_cast<unsigned>(ceil_div(B, kPriorRows))),
                     dim3(kPriorRows), lds, st, T, d, seed, sid, offset, B, theta);
  ABC_LAUNCH_CHECK("prior_rvs_kernel");
  return kOk;
}

}  // extern "C"

namespace abc {
int preload_prior() { return preload_kernel(prior_logpdf_kernel); }
}  // namespace abc
