// Exact-inference ABC: the count-data kernels, fused with
// the stochastic acceptance.
//
// replaces BinomialKernel / PoissonKernel / NegativeBinomialKernel.__call__,
// distance/kernel.py:365-537 (SCALE_LOG), i.e. scipy.stats logpmf summed over
// the statistics s with n = trunc(stats_T[s][b]), k = trunc(x0[s]):
//   binomial (3): lf(n) - lf(k) - lf(n-k) + xlogy(k, p) + xlog1py(n-k, -p)
//   Poisson  (4): xlogy(k, n) - n - lf(k)
//   negbin   (5): lf(k+n-1) - lf(k) - lf(n-1) + n log p + xlog1py(k, -p)
// lf(m) = lgamma(m + 1) (logfact.hpp).
//
// The design exists to keep transcendentals and roundings out of the
// per-element work.  Regrouped over s:
//   binomial: sum [lf(n) - lf(n-k)] + log1p(-p) sum (n-k) + C
//   Poisson : sum k log n           -           sum n     + C
//   negbin  : sum [lf(k+n-1) - lf(n-1)] + log p sum n     + C
// C = sum of the terms in k alone (-lf(k) + k log p, ...) is the same for
// every evaluation: each block computes it once, in double-double, with a
// fixed 256-way split and tree.  The counts multiply log p / log1p(-p) only
// as an integer sum (exact below 2^53).  What is left per element is two
// table reads and a compensated add (binomial, negbin) or one table read and
// one fma (Poisson).
//
// Tables.  lf(m) for m < T = 4096 (Poisson: log m) is staged into LDS once
// per block, 32 KiB; blocks are persistent (grid <= kCountGrid) and serve
// passes of 256 evaluations grid-stride, so the staging is amortised.  The
// truncated k_s sit in LDS in chunks of kStatChunk statistics: a wave reads
// them as a broadcast.  Counts >= T take the Stirling series (the Poisson
// kernel: the device log); that code is entered only when a wave vote says a
// lane needs it, and only those lanes take its value, so a wave of small
// counts issues no transcendental and a lane's result never depends on its
// wave-mates.
//
// Order and error.  One lane owns one evaluation and walks s = 0..S-1 over
// coalesced stat-major rows.  The lf differences are accumulated with TwoSum
// compensation and combined with the product and C in double-double, rounded
// once: per term the error is the table's (<= 1 ulp), the Stirling branch's
// (<= 3.43 2^-53, logfact.hpp) or the host logarithm's, plus one final
// rounding; the integer sums and the Poisson fma chain round once per
// statistic.  pd[b] depends on column b, x0, p and the kind only.
//
// Out of support, as scipy: NaN when the statistic is not finite, |x| >= 2^52,
// n < 0 (binomial, Poisson), n <= 0 or p = 0 (negbin); otherwise -inf when
// k < 0, k > n, or a nonzero count meets log 0; a zero count times log 0 is 0.
// Out-of-support lanes walk on with a stand-in count of 0 and are overridden
// at the end, so no infinity or NaN ever enters the arithmetic.
#include "common.hpp"
#include "logfact.hpp"
#include "philox.hpp"
#include "stochastic_common.hpp"

namespace abc {

namespace {

// 32 KiB table + 6 KiB chunk + the vote's scratch = 39168 B: four blocks per
// CU (160 KiB), and the grid is capped at one such wave of blocks on 256 CUs
constexpr int kCountGrid = 1024;
constexpr int kStatChunk = 768;    // truncated k_s held in LDS at a time (>= 512)
constexpr double kTwo52 = 4503599627370496.0;

// lf(m) of an integer-valued 0 <= m: LDS table below T, Stirling above; the
// Stirling code runs only in waves where some lane needs it
__device__ inline double lf_lookup(double m, const double* tab) {
  const bool big = m >= kLfTable;
  double r = tab[big ? 0 : static_cast<int>(m)];
  if (__ballot(big) != 0) {
    if (big) r = lf_stirling(m);
  }
  return r;
}

// log(m) of an integer-valued 0 <= m (entry 0 is 0, see log_table_entry)
__device__ inline double log_lookup(double m, const double* tab) {
  const bool big = m >= kLfTable;
  double r = tab[big ? 0 : static_cast<int>(m)];
  if (__ballot(big) != 0) {
    if (big) r = log(m);
  }
  return r;
}

}  // namespace

__global__ __launch_bounds__(256) void count_table_init_kernel(
    double* __restrict__ table) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= kLfTable) return;
  table[m] = lf_table_entry(m);
  table[kLfTable + m] = log_table_entry(m);
}

// KIND 3: binomial, 4: Poisson, 5: negative binomial
template <int KIND>
__global__ __launch_bounds__(256) void count_kernel_kernel(
    const double* __restrict__ stats_T, int64_t ld,
    const double* __restrict__ x0, int S, double log_p, double log1m_p,
    const double* __restrict__ table, int64_t B, double* __restrict__ pd_out,
    // fused acceptance (accept == nullptr: density only)
    double pdf_norm, double inv_temp, int apply_iw,
    const double* __restrict__ u_in, uint64_t seed, uint64_t stream,
    uint64_t offset, uint8_t* __restrict__ accept, double* __restrict__ accw,
    uint8_t* __restrict__ guard) {
#pragma clang fp contract(off)
  __shared__ double tab[kLfTable];
  __shared__ double ks[kStatChunk];  // first the reduction scratch of C
  const int tid = threadIdx.x;

  for (int i = tid; i < kLfTable; i += 256)
    tab[i] = table[(KIND == 4 ? kLfTable : 0) + i];

  // ---- the terms in k alone: C, and what k and p already decide ------------
  // log of the probability that multiplies k, and of the one that multiplies
  // the simulated counts
  const double log_k = KIND == 3 ? log_p : log1m_p;
  const double log_n = KIND == 3 ? log1m_p : log_p;
  const bool log_k_fin = log_k > -INFINITY, log_n_fin = log_n > -INFINITY;
  dd part{0.0, 0.0};
  int cflag = 0;  // bit 0: NaN, bit 1: -inf
  for (int s = tid; s < S; s += 256) {
    const double xs = x0[s];
    const bool ok = fabs(xs) < kTwo52;
    const double k = trunc(xs);
    if (!ok) cflag |= 1;
    if (ok && k < 0.0) cflag |= 2;
    if (ok && k > 0.0) {
      const double lfk = k < kLfTable ? table[static_cast<int>(k)] : lf_stirling(k);
      part = dd_add(part, dd{-lfk, 0.0});
      if (KIND != 4) {
        if (log_k_fin)
          part = dd_add(part, two_prod(k, log_k));
        else
          cflag |= 2;
      }
    }
  }
  if (KIND == 5 && !log_n_fin) cflag |= 1;  // scipy: nbinom needs p > 0
  ks[2 * tid] = part.hi;
  ks[2 * tid + 1] = part.lo;
  // block votes (any thread), which also order the LDS writes above
  const bool c_nan = __syncthreads_or(cflag & 1) != 0;
  const bool c_inf = __syncthreads_or(cflag & 2) != 0;
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      const dd r = dd_add(dd{ks[2 * tid], ks[2 * tid + 1]},
                          dd{ks[2 * (tid + w)], ks[2 * (tid + w) + 1]});
      ks[2 * tid] = r.hi;
      ks[2 * tid + 1] = r.lo;
    }
    __syncthreads();
  }
  const dd C{ks[0], ks[1]};
  const double log_n_use = log_n_fin ? log_n : 0.0;

  // ---- passes of 256 evaluations -------------------------------------------
  const int64_t npass = ceil_div(B, 256);
  bool staged = false;
  for (int64_t pass = blockIdx.x; pass < npass; pass += gridDim.x) {
    const int64_t b = pass * 256 + tid;
    const bool bv = b < B;
    const double* col = stats_T + (bv ? b : 0);
    double acc = 0.0, comp = 0.0, cnt = 0.0;
    bool f_nan = false, f_inf = false;
    for (int c0 = 0; c0 < S; c0 += kStatChunk) {
      const int cs = min(kStatChunk, S - c0);
      if (!staged || S > kStatChunk) {
        __syncthreads();  // C and the previous chunk have been read
        for (int i = tid; i < cs; i += 256) ks[i] = trunc(x0[c0 + i]);
        __syncthreads();
        staged = true;
      }
      for (int i = 0; i < cs; ++i) {
        // a lane without a column walks the stand-in count 1
        const double x = bv ? col[static_cast<int64_t>(c0 + i) * ld] : 1.0;
        const double k = ks[i];
        const double n = trunc(x);
        const bool ok = fabs(x) < kTwo52;
        if (KIND == 3) {
          const double nk = n - k;
          const bool in = ok && n >= 0.0;
          f_nan |= !in;
          f_inf |= nk < 0.0;
          const bool good = in && nk >= 0.0 && k >= 0.0;
          const double hi = good ? n : 0.0, lo = good ? nk : 0.0;
          dd t = two_sum(acc, lf_lookup(hi, tab));
          comp += t.lo;
          t = two_sum(t.hi, -lf_lookup(lo, tab));
          comp += t.lo;
          acc = t.hi;
          cnt += lo;
        } else if (KIND == 4) {
          const bool in = ok && n >= 0.0;
          f_nan |= !in;
          f_inf |= k > 0.0 && n == 0.0;
          const bool good = in && k > 0.0;
          acc = fma(good ? k : 0.0, log_lookup(good ? n : 0.0, tab), acc);
          cnt += in ? n : 0.0;
        } else {
          const bool in = ok && n >= 1.0;
          f_nan |= !in;
          const bool good = in && k >= 0.0;
          const double lo = good ? n - 1.0 : 0.0, hi = good ? k + lo : 0.0;
          dd t = two_sum(acc, lf_lookup(hi, tab));
          comp += t.lo;
          t = two_sum(t.hi, -lf_lookup(lo, tab));
          comp += t.lo;
          acc = t.hi;
          cnt += in ? n : 0.0;
        }
      }
    }
    if (!bv) continue;
    dd tot = two_sum(acc, comp);
    if (KIND == 4) {
      tot = dd_add(tot, dd{-cnt, 0.0});
    } else {
      if (!log_n_fin && cnt > 0.0) f_inf = true;
      tot = dd_add(tot, two_prod(cnt, log_n_use));
    }
    tot = dd_add(tot, C);
    double pd = tot.hi;
    if (f_inf || c_inf) pd = -INFINITY;
    if (f_nan || c_nan) pd = NAN;
    pd_out[b] = pd;
    if (accept) {
      const double u = u_in ? u_in[b] : philox_u01(seed, stream, offset + b);
      uint8_t a, g;
      double w;
      stochastic_decide(pd, pdf_norm, inv_temp, 1, apply_iw, u, a, w, g);
      accept[b] = a;
      if (accw) accw[b] = w;
      if (guard) guard[b] = g;
    }
  }
}

}  // namespace abc

using namespace abc;

extern "C" {

size_t abc_count_table_bytes(void) { return 2 * kLfTable * sizeof(double); }

int abc_count_table_init_f64(double* table, hipStream_t st) {
  ABC_REQUIRE(table, "count_table_init: null pointer");
  hipLaunchKernelGGL(count_table_init_kernel, dim3(kLfTable / 256), dim3(256),
                     0, st, table);
  ABC_LAUNCH_CHECK("count_table_init_kernel");
  return kOk;
}

int abc_count_kernel_f64(const double* stats_T, int64_t ld, const double* x0,
                         int S, int kind, double p, double log_p,
                         double log1m_p, const double* table, int64_t B,
                         double* pd_out, double pdf_norm, double inv_temp,
                         int apply_iw, const double* u, uint64_t seed,
                         uint64_t stream, uint64_t offset, uint8_t* accept,
                         double* accw, uint8_t* guard, hipStream_t st) {
  ABC_REQUIRE(B >= 0 && S >= 1 && ld >= B, "count_kernel: bad sizes");
  ABC_REQUIRE(S <= kMaxStats, "count_kernel: S > %d unsupported", kMaxStats);
  ABC_REQUIRE(kind >= 3 && kind <= 5,
              "count_kernel: kind must be 3 (binomial), 4 (poisson) or 5 "
              "(negative binomial)");
  ABC_REQUIRE(kind == 4 || (p >= 0.0 && p <= 1.0),
              "count_kernel: p must be in [0, 1]");
  if (B == 0) return kOk;
  ABC_REQUIRE(stats_T && x0 && table && pd_out, "count_kernel: null pointer");
  const dim3 g(stream_grid(B, 256, kCountGrid)), blk(256);
#define ABC_CK_LAUNCH(KIND)                                                   \
  hipLaunchKernelGGL(count_kernel_kernel<KIND>, g, blk, 0, st, stats_T, ld,   \
                     x0, S, log_p, log1m_p, table, B, pd_out, pdf_norm,       \
                     inv_temp, apply_iw, u, seed, stream, offset, accept,     \
                     accw, guard)
  if (kind == 3)
    ABC_CK_LAUNCH(3);
  else if (kind == 4)
    ABC_CK_LAUNCH(4);
  else
    ABC_CK_LAUNCH(5);
#undef ABC_CK_LAUNCH
  ABC_LAUNCH_CHECK("count_kernel_kernel");
  return kOk;
}

}  // extern "C"

namespace abc {
int preload_stochastic_count() { return preload_kernel(count_kernel_kernel<3>); }
}  // namespace abc
