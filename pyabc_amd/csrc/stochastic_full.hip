// Exact-inference ABC: the full-covariance normal kernel
// on the fp64 matrix cores, fused with the stochastic acceptance.
//
// replaces NormalKernel.__call__, distance/kernel.py:173-194
//   log pd = scipy.stats.multivariate_normal(cov).logpdf(x - x_0)
//          = -0.5 * (rank log(2 pi) + log_pdet + |(x - x_0) U|^2)
// with U the scipy _PSD whitening factor (host, kernels.psd_whitening) and
// c = rank log(2 pi) + log_pdet a host scalar.  Over a round of B evaluations
// the quadratic form is the GEMM  Y[r][b] = sum_s U[s][r] diff[s][b]  with a
// fused column norm, 2 S R FLOP per evaluation, on v_mfma_f64_16x16x4_f64.
//
// Work split.  A 256-thread block owns 64 consecutive evaluations, 16 per
// wave.  One MFMA is D[16 components][16 evaluations] += A[16 x 4] B[4 x 16]
// over 4 statistics:
//   A (lane l: row l % 16, k = l / 16) = U[k0 + l/16][r0 + l%16]   from LDS,
//   B (lane l: k = l / 16, col l % 16) = stats_T[(k0 + l/16) ld + b0 + l%16]
//                                        - x0[k0 + l/16]           from HBM.
// The stat-major statistics need no transpose: the 16 evaluations of a tile
// are 16 consecutive doubles of one row (128-byte segments).  The evaluations
// are the COLUMNS of D, so lane l holds, in its four accumulator values per
// tile, four components of evaluation l % 16: the squared norm is summed
// inside the lane (whichever rows the four values are) and only two shuffles
// (xor 16, 32) finish it.
//
// U through LDS.  All four waves use the same U.  It is staged in chunks of
// kKT = 16 statistics x RB = 16 NT components (NT = 1, 2, 4, 8 tiles, the
// smallest that covers R, at most 128 components), double-buffered: the next
// chunk's U values and the wave's next diffs are loaded into registers before
// the chunk's MFMAs and written to the other LDS buffer after them, one
// barrier per chunk.  Rows are padded to an odd multiple of 128 bytes so the
// four statistics rows of one ds_read_b64 fall on different banks.  For
// R > 128 the r-blocks run one after another and re-read the diffs (8 S bytes
// per evaluation, L2-resident).
//
// Order.  Per r-block the accumulators are squared and added in tile, then
// register order; r-blocks in order; then the fixed xor tree.  pd[b] is a
// function of column b, x0, U and c alone: no value depends on B, ld or the
// column's place in a tile, wave or block (padding rows, components and
// columns are exact zeros).
//
// Tails: statistics rows >= S and components >= R are zero-filled in LDS and
// in the diffs, columns >= B are not loaded (ld may equal B) and not stored.
#include "common.hpp"
#include "philox.hpp"
#include "stochastic_common.hpp"

namespace abc {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kKT = 16;        // statistics per LDS chunk (4 MFMA k-steps)
constexpr int kMaxComp = 4096; // whitened components
constexpr int kEvalsPerBlock = 64;

}  // namespace

template <int NT>
__global__ __launch_bounds__(256) void normal_kernel_kernel(
    const double* __restrict__ stats_T, int64_t ld,
    const double* __restrict__ x0, const double* __restrict__ U, int S, int R,
    double c, int64_t B, double* __restrict__ pd_out,
    // fused acceptance (accept == nullptr: density only)
    double pdf_norm, double inv_temp, int apply_iw,
    const double* __restrict__ u_in, uint64_t seed, uint64_t stream,
    uint64_t offset, uint8_t* __restrict__ accept, double* __restrict__ accw,
    uint8_t* __restrict__ guard) {
  constexpr int RB = 16 * NT;                        // components per r-block
  constexpr int LDW = RB + (RB % 32 == 0 ? 16 : 0);  // LDS row, doubles
  constexpr int KSTEPS = kKT / 4;
  __shared__ double lds[2][kKT * LDW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, j = lane & 15;
  const int64_t b =
      static_cast<int64_t>(blockIdx.x) * kEvalsPerBlock + wave * 16 + j;
  const bool bv = b < B;
  const double* col = stats_T + (bv ? b : 0);

  const int nkc = (S + kKT - 1) / kKT;
  const int nch = nkc * ((R + RB - 1) / RB);

  double ureg[NT];      // this thread's share of the next U chunk
  double dnext[KSTEPS]; // this lane's diffs of the next chunk
  // chunk (k0, r0): U[k0 .. k0+16)[r0 .. r0+RB) and diff rows k0 .. k0+16
  auto load_chunk = [&](int k0, int r0) {
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int e = tid + 256 * i;
      const int s = k0 + e / RB, r = r0 + e % RB;
      ureg[i] = (s < S && r < R) ? U[static_cast<int64_t>(s) * R + r] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < KSTEPS; ++q) {
      const int s = k0 + 4 * q + g;
      dnext[q] = (bv && s < S) ? col[static_cast<int64_t>(s) * ld] - x0[s] : 0.0;
    }
  };
  auto store_chunk = [&](double* buf) {
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int e = tid + 256 * i;
      buf[(e / RB) * LDW + e % RB] = ureg[i];
    }
  };

  d4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  double part = 0.0;

  int k0 = 0, r0 = 0, kc = 0;
  load_chunk(0, 0);
  store_chunk(lds[0]);
  __syncthreads();
  for (int ch = 0; ch < nch; ++ch) {
    const double* cur = lds[ch & 1];
    double dcur[KSTEPS];
#pragma unroll
    for (int q = 0; q < KSTEPS; ++q) dcur[q] = dnext[q];
    const bool more = ch + 1 < nch;
    const bool last_k = kc + 1 == nkc;
    if (more) {
      if (last_k) { k0 = 0; r0 += RB; } else { k0 += kKT; }
      load_chunk(k0, r0);
    }
#pragma unroll
    for (int q = 0; q < KSTEPS; ++q) {
      const double* row = cur + (4 * q + g) * LDW + j;
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[16 * t], dcur[q],
                                                      acc[t], 0, 0, 0);
    }
    // the other buffer was last read before the previous barrier
    if (more) store_chunk(lds[(ch + 1) & 1]);
    __syncthreads();
    if (last_k) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          part = fma(acc[t][v], acc[t][v], part);
          acc[t][v] = 0.0;
        }
      }
      kc = 0;
    } else {
      ++kc;
    }
  }
  part += __shfl_xor(part, 16, 64);
  part += __shfl_xor(part, 32, 64);

  if (g != 0 || !bv) return;
  const double pd = -0.5 * (c + part);
  pd_out[b] = pd;
  if (accept) {
    const double u = u_in ? u_in[b] : philox_u01(seed, stream, offset + b);
    uint8_t a, gd;
    double w;
    stochastic_decide(pd, pdf_norm, inv_temp, 1, apply_iw, u, a, w, gd);
    accept[b] = a;
    if (accw) accw[b] = w;
    if (guard) guard[b] = gd;
  }
}

}  // namespace abc

using namespace abc;

extern "C" {

int abc_normal_kernel_f64(const double* stats_T, int64_t ld, const double* x0,
                          const double* U, int S, int R, double c, int64_t B,
                          double* pd_out, double pdf_norm, double inv_temp,
                          int apply_iw, const double* u, uint64_t seed,
                          uint64_t stream, uint64_t offset, uint8_t* accept,
                          double* accw, uint8_t* guard, hipStream_t st) {
  ABC_REQUIRE(B >= 0 && S >= 1 && R >= 1 && ld >= B,
              "normal_kernel: bad sizes");
  ABC_REQUIRE(S <= kMaxStats, "normal_kernel: S > %d unsupported", kMaxStats);
  ABC_REQUIRE(R <= kMaxComp, "normal_kernel: R > %d unsupported", kMaxComp);
  if (B == 0) return kOk;
  ABC_REQUIRE(stats_T && x0 && U && pd_out, "normal_kernel: null pointer");
  const int64_t grid = ceil_div(B, kEvalsPerBlock);
  ABC_REQUIRE(grid <= 0x7fffffff, "normal_kernel: B too large for one launch");
  const dim3 g(static_cast<unsigned>(grid)), blk(256);
#define ABC_NK_LAUNCH(NT)                                                     \
  hipLaunchKernelGGL(normal_kernel_kernel<NT>, g, blk, 0, st, stats_T, ld,    \
                     x0, U, S, R, c, B, pd_out, pdf_norm, inv_temp, apply_iw, \
                     u, seed, stream, offset, accept, accw, guard)
  if (R <= 16)
    ABC_NK_LAUNCH(1);
  else if (R <= 32)
    ABC_NK_LAUNCH(2);
  else if (R <= 64)
    ABC_NK_LAUNCH(4);
  else
    ABC_NK_LAUNCH(8);
#undef ABC_NK_LAUNCH
  ABC_LAUNCH_CHECK("normal_kernel_kernel");
  return kOk;
}

}  // extern "C"

namespace abc {
int preload_stochastic_full() { return preload_kernel(normal_kernel_kernel<1>); }
}  // namespace abc
