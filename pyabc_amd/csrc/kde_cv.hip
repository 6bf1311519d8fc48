// Cross-validated KDE log-likelihood for a grid of bandwidth scalings: the
// device part of GridSearchCV over MultivariateNormalTransition.scaling.
//
// replaces sklearn's GridSearchCV driving, per fold f and grid value s_g,
//   MultivariateNormalTransition(scaling=s_g).fit(X_train, w_train)
//   Transition.score(X_test, w_test) = sum_i w_i log pdf(x_i)
//                     transition/model_selection.py:9-69, base.py:106-107,
//                     multivariatenormal.py:67-85, 102-125
// The fold covariance is cov_f(s) = cov_f(1) s, so with z = (x - mu_f) U_f
// whitened by cov_f(1) every pair (test row i of fold f, training row j) has
// ONE squared distance q = |z_i - z_j|^2 and G exponents
//   t_g = lw2_j - coef[g] q,   lw2_j = log2 w_j,  coef[g] = log2(e) / (2 s_g).
// out_L[g][i] = ln sum_{j not in fold(i)} 2^t_g; the host adds the Gaussian
// constant.  k G fits and k G density passes of the reference become one pass
// over the n^2 (k-1)/k pairs with the d-dimensional part done once.
//
// Kernels.
//  1. kde_cv_whiten_kernel: Z[f][j][DP] = (x_j - mu_f) U_f for every fold f and
//     every row j (DP = d padded to 4, 8, 16 or 32, zero filled), NRM[f][j] =
//     |z|^2, LW2[j] = log2 w_j (-inf for w_j = 0).  k n DP doubles written once
//     (32 MB at n = 1e5, d = 8, k = 5) against n^2 (k-1)/k pair evaluations:
//     whitening while staging would redo the d x d product once per row tile.
//  2. kde_cv_kernel<KS, GN>: a 256-thread block owns 64 test rows of one fold
//     (16 per wave) and one segment of that fold's training columns.  The
//     training columns of fold [lo, hi) are addressed by a dense index
//     c in [0, n - (hi - lo)): row c for c < lo, row c + (hi - lo) otherwise,
//     so no tile straddles the fold and only the last chunk has a masked tail
//     (z = 0, lw2 = -inf: contributes exactly nothing).
//     Pair geometry on v_mfma_f64_16x16x4_f64:  D[training 16][test 16] +=
//     A[16 x 4] B[4 x 16] over 4 whitened components,
//       A (lane l: row l % 16, k = l / 16) = training tile, from LDS,
//       B (lane l: k = l / 16, col l % 16) = the wave's test rows, in registers
//         for the whole kernel (KS = DP / 4 doubles per lane) with |z_i|^2.
//     Lane l then holds D[4 v + l / 16][l % 16], v < 4: four training columns
//     of ONE test row, q = |z_i|^2 + |z_j|^2 - 2 D (clamped at 0).  Training
//     columns move in chunks of 64 (four MFMA tiles) through double-buffered
//     LDS: the next chunk is loaded into registers before the chunk's MFMAs and
//     stored to the other buffer after its fan-out, one barrier per chunk.  LDS
//     rows are DP + 2 doubles: the 32 lanes of a ds_read_b64 half fall on 32
//     different 8-byte banks.
//     Fan-out.  A lane holds 16 pairs of its test row per chunk.  Per grid
//     value: t = fma(-coef[g], q, lw2_j) in fp64, the running maximum of the
//     FULL exponent (log-weight included) is updated once per chunk, the terms
//     2^(t - m) go through v_exp_f32 and are summed in fp32 over the 16 pairs,
//     then added to the fp64 running sum.  The running maximum is kept as an
//     INTEGER (ceil of the largest exponent seen), so the rescale of the sum is
//     an exact ldexp: no rescale exponential at all (the flash-attention form
//     spends one per (row, g) per tile and compounds one rounding per rescale,
//     ~n / 64 roundings in the worst case of an ever-growing maximum).  Terms
//     are in (0, 1] with the largest above 1/2: nothing depends on the weights'
//     dynamic range or on how far a test row lies from the training set.
//     The four lanes of a test row (l / 16 = 0..3) keep separate (m, s), merged
//     at the end by two xor shuffles (symmetric, so order-free), and lane
//     group 0 writes the segment partial (m, s) per (row, g).
//  3. kde_cv_merge_kernel: one block per (fold, g) merges the NSEG partials of
//     each of the fold's rows in segment order (ldexp to the common integer
//     maximum, exact), writes out_L and reduces w_i out_L[g][i] with a fixed
//     strided order and tree.
// The segment count is a function of n and k only (cv_segments) and the
// chunks of a segment a function of the fold: results are bit-identical from
// run to run and independent of any launch shape.
//
// Error of out_L (DESIGN.md "GridSearchCV"): the exponent t is fp64 (~1e-15 |z|^2
// from the expansion's cancellation), t - m is rounded to fp32 (relative 2^-24
// of a value whose term is 2^-(m-t): at most 2^-24 * 0.53 on the sum), v_exp_f32
// is 1 ulp (1.2e-7), and the fp32 sum of 16 non-negative terms adds at most
// 15 * 2^-24 = 8.9e-7: |dL| <= 1.1e-6 in the worst case, ~1e-7 typically.
#include "common.hpp"

namespace abc {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kMaxD = 32;
constexpr int kMaxG = 8;        // grid values per launch
constexpr int kRows = 64;       // test rows per block (16 per wave)
constexpr int kChunk = 64;      // training columns per LDS chunk (4 tiles)
constexpr int kMaxSeg = 32;
constexpr double kNoMax = -1e30;  // "no term yet" (any double this large is an integer)

inline int cv_dpad(int d) { return d <= 4 ? 4 : d <= 8 ? 8 : d <= 16 ? 16 : 32; }

// column segments: enough blocks for the chip at small n, a function of
// (n, k) alone
inline int cv_segments(int64_t n, int k) {
  const int64_t tiles = ceil_div(n, kRows) + k;
  int64_t s = 2048 / tiles;
  const int64_t chunks = ceil_div(n, kChunk);
  if (s > chunks) s = chunks;
  if (s > kMaxSeg) s = kMaxSeg;
  return s < 1 ? 1 : static_cast<int>(s);
}

struct CvLayout {
  size_t off_fold, off_lw2, off_nrm, off_z, off_pm, off_ps, total;
};

inline CvLayout cv_layout(int64_t n, int d, int k, int G) {
  auto up = [](size_t b) { return (b + 255) & ~static_cast<size_t>(255); };
  const size_t nseg = cv_segments(n, k), dp = cv_dpad(d);
  CvLayout L;
  size_t o = 0;
  L.off_fold = o; o += up(sizeof(int64_t) * (k + 1));
  L.off_lw2 = o;  o += up(sizeof(double) * n);
  L.off_nrm = o;  o += up(sizeof(double) * n * k);
  L.off_z = o;    o += up(sizeof(double) * n * k * dp);
  L.off_pm = o;   o += up(sizeof(double) * n * G * nseg);
  L.off_ps = o;   o += up(sizeof(double) * n * G * nseg);
  L.total = o;
  return L;
}

}  // namespace

__global__ __launch_bounds__(256) void kde_cv_whiten_kernel(
    const double* __restrict__ X, const double* __restrict__ w, int64_t n, int d,
    int DP, const double* __restrict__ mu, const double* __restrict__ Us,
    double* __restrict__ Z, double* __restrict__ NRM, double* __restrict__ LW2) {
  const int f = blockIdx.y;
  const int64_t j = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (j >= n) return;
  const double* x = X + j * d;
  const double* m = mu + static_cast<int64_t>(f) * d;
  const double* U = Us + static_cast<int64_t>(f) * d * d;
  double* z = Z + (static_cast<int64_t>(f) * n + j) * DP;
  double nrm = 0.0;
  for (int c = 0; c < d; ++c) {
    double a = 0.0;
    for (int r = 0; r < d; ++r) a = fma(x[r] - m[r], U[r * d + c], a);
    z[c] = a;
    nrm = fma(a, a, nrm);
  }
  for (int c = d; c < DP; ++c) z[c] = 0.0;
  NRM[static_cast<int64_t>(f) * n + j] = nrm;
  if (f == 0) LW2[j] = log2(w[j]);   // log2(0) = -inf: the row contributes nothing
}

template <int KS, int GN>
__global__ __launch_bounds__(256) void kde_cv_kernel(
    const double* __restrict__ Z, const double* __restrict__ NRM,
    const double* __restrict__ LW2, int64_t n, const int64_t* __restrict__ fold_off,
    const double* __restrict__ coef, int nseg, double* __restrict__ PM,
    double* __restrict__ PS) {
  constexpr int DP = 4 * KS;
  constexpr int LDW = DP + 2;
  __shared__ double zs[2][kChunk * LDW];
  __shared__ double ns[2][kChunk];
  __shared__ double ls[2][kChunk];

  const int f = blockIdx.y, seg = blockIdx.z;
  const int64_t lo = fold_off[f], hi = fold_off[f + 1], nf = hi - lo;
  const int64_t row0 = lo + static_cast<int64_t>(blockIdx.x) * kRows;
  if (row0 >= hi) return;   // block-uniform: before any barrier
  const int64_t T = n - nf;                        // training columns
  const int64_t nch = ceil_div(T, kChunk);
  const int64_t cps = ceil_div(nch, nseg);
  const int64_t c0 = seg * cps;
  const int64_t c1 = c0 + cps < nch ? c0 + cps : nch;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g4 = lane >> 4, j = lane & 15;
  const double* Zf = Z + static_cast<int64_t>(f) * n * DP;
  const double* Nf = NRM + static_cast<int64_t>(f) * n;

  const int64_t i = row0 + wave * 16 + j;
  const bool iv = i < hi;
  double breg[KS];
#pragma unroll
  for (int q = 0; q < KS; ++q) breg[q] = iv ? Zf[i * DP + 4 * q + g4] : 0.0;
  const double ni = iv ? Nf[i] : 0.0;

  double cf[GN], m[GN], s[GN];
#pragma unroll
  for (int g = 0; g < GN; ++g) {
    cf[g] = coef[g];
    m[g] = kNoMax;
    s[g] = 0.0;
  }

  // staging: thread tid carries elements tid + 256 u of the chunk's 64 x DP
  // block, and threads < 64 the column's norm and log-weight
  double zreg[KS], nreg = 0.0, lreg = 0.0;
  auto load_chunk = [&](int64_t c) {
#pragma unroll
    for (int u = 0; u < KS; ++u) {
      const int e = tid + 256 * u;
      const int64_t vc = c * kChunk + e / DP;
      const int64_t r = vc < lo ? vc : vc + nf;
      zreg[u] = vc < T ? Zf[r * DP + e % DP] : 0.0;
    }
    if (tid < kChunk) {
      const int64_t vc = c * kChunk + tid;
      const int64_t r = vc < lo ? vc : vc + nf;
      const bool ok = vc < T;
      nreg = ok ? Nf[r] : 0.0;
      lreg = ok ? LW2[r] : -INFINITY;
    }
  };
  auto store_chunk = [&](int b) {
#pragma unroll
    for (int u = 0; u < KS; ++u) {
      const int e = tid + 256 * u;
      zs[b][(e / DP) * LDW + e % DP] = zreg[u];
    }
    if (tid < kChunk) {
      ns[b][tid] = nreg;
      ls[b][tid] = lreg;
    }
  };

  if (c0 < c1) {
    load_chunk(c0);
    store_chunk(0);
  }
  __syncthreads();
  for (int64_t c = c0; c < c1; ++c) {
    const int b = static_cast<int>(c - c0) & 1;
    const bool more = c + 1 < c1;
    if (more) load_chunk(c + 1);

    double q[16], lw[16];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      d4 acc = d4{0.0, 0.0, 0.0, 0.0};
      const double* row = &zs[b][(16 * t + j) * LDW + g4];
#pragma unroll
      for (int k4 = 0; k4 < KS; ++k4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(row[4 * k4], breg[k4], acc,
                                                   0, 0, 0);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int col = 16 * t + 4 * v + g4;
        q[4 * t + v] = fmax(fma(-2.0, acc[v], ni + ns[b][col]), 0.0);
        lw[4 * t + v] = ls[b][col];
      }
    }
#pragma unroll
    for (int g = 0; g < GN; ++g) {
      double tmax = -INFINITY;
#pragma unroll
      for (int p = 0; p < 16; ++p) tmax = fmax(tmax, fma(-cf[g], q[p], lw[p]));
      const double mn = fmax(m[g], ceil(tmax));
      s[g] = ldexp(s[g], static_cast<int>(fmax(m[g] - mn, -2100.0)));
      m[g] = mn;
      float ps = 0.0f;
#pragma unroll
      for (int p = 0; p < 16; ++p)
        ps += __builtin_amdgcn_exp2f(
            static_cast<float>(fma(-cf[g], q[p], lw[p]) - mn));
      s[g] += static_cast<double>(ps);
    }
    // the other buffer was last read before the previous barrier
    if (more) store_chunk(b ^ 1);
    __syncthreads();
  }

  // the four lanes of a test row: symmetric merges, every lane ends equal
#pragma unroll
  for (int g = 0; g < GN; ++g) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const double mo = __shfl_xor(m[g], o, 64);
      const double so = __shfl_xor(s[g], o, 64);
      const double mm = fmax(m[g], mo);
      s[g] = ldexp(s[g], static_cast<int>(fmax(m[g] - mm, -2100.0))) +
             ldexp(so, static_cast<int>(fmax(mo - mm, -2100.0)));
      m[g] = mm;
    }
  }
  if (g4 == 0 && iv) {
#pragma unroll
    for (int g = 0; g < GN; ++g) {
      const int64_t o = (static_cast<int64_t>(seg) * GN + g) * n + i;
      PM[o] = m[g];
      PS[o] = s[g];
    }
  }
}

// one block per (fold, g): out_L of the fold's rows and the fold's score
__global__ __launch_bounds__(256) void kde_cv_merge_kernel(
    const double* __restrict__ PM, const double* __restrict__ PS,
    const double* __restrict__ w, int64_t n, const int64_t* __restrict__ fold_off,
    int G, int nseg, double* __restrict__ out_L, double* __restrict__ out_score) {
  __shared__ double red[4];
  const int f = blockIdx.x, g = blockIdx.y;
  const int64_t lo = fold_off[f], hi = fold_off[f + 1];
  double part = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    double M = kNoMax;
    for (int sg = 0; sg < nseg; ++sg)
      M = fmax(M, PM[(static_cast<int64_t>(sg) * G + g) * n + i]);
    double S = 0.0;
    for (int sg = 0; sg < nseg; ++sg) {
      const int64_t o = (static_cast<int64_t>(sg) * G + g) * n + i;
      S += ldexp(PS[o], static_cast<int>(fmax(PM[o] - M, -2100.0)));
    }
    // S = 0 (no training weight reaches the row): log2 -> -inf, as numpy's log
    const double L = (M + log2(S)) * 0.6931471805599453;
    out_L[static_cast<int64_t>(g) * n + i] = L;
    part += w[i] * L;
  }
  part = block_sum<double, 256>(part, red);
  if (threadIdx.x == 0) out_score[static_cast<int64_t>(f) * G + g] = part;
}

}  // namespace abc

using namespace abc;

extern "C" {

size_t abc_kde_cv_workspace_bytes(int64_t n, int d, int k, int G) {
  if (n < 1 || d < 1 || d > kMaxD || k < 1 || G < 1 || G > kMaxG) return 0;
  return cv_layout(n, d, k, G).total;
}

int abc_kde_cv_f64(const double* X, const double* w, int64_t n, int d,
                   const int64_t* fold_off, int k, const double* mu,
                   const double* Us, const double* coef, int G, double* out_L,
                   double* out_score, void* ws, size_t ws_bytes,
                   hipStream_t st) {
  ABC_REQUIRE(n >= 2 && d >= 1 && k >= 2 && k <= n, "kde_cv: bad sizes");
  ABC_REQUIRE(d <= kMaxD, "kde_cv: d > %d unsupported", kMaxD);
  ABC_REQUIRE(G >= 1 && G <= kMaxG, "kde_cv: G must be 1..%d per call", kMaxG);
  ABC_REQUIRE(k <= 65535, "kde_cv: more than 65535 folds");
  ABC_REQUIRE(fold_off, "kde_cv: null fold_off");
  ABC_REQUIRE(fold_off[0] == 0 && fold_off[k] == n,
              "kde_cv: fold_off must run from 0 to n");
  int64_t max_nf = 0;
  for (int f = 0; f < k; ++f) {
    const int64_t nf = fold_off[f + 1] - fold_off[f];
    ABC_REQUIRE(nf >= 1 && nf < n, "kde_cv: fold %d is empty or everything", f);
    if (nf > max_nf) max_nf = nf;
  }
  ABC_REQUIRE(X && w && mu && Us && coef && out_L && out_score && ws,
              "kde_cv: null pointer");
  const CvLayout L = cv_layout(n, d, k, G);
  ABC_REQUIRE(ws_bytes >= L.total, "kde_cv: workspace too small");
  ABC_REQUIRE(ceil_div(n, 256) <= 0x7fffffff, "kde_cv: n too large");

  char* base = static_cast<char*>(ws);
  int64_t* fo = reinterpret_cast<int64_t*>(base + L.off_fold);
  double* LW2 = reinterpret_cast<double*>(base + L.off_lw2);
  double* NRM = reinterpret_cast<double*>(base + L.off_nrm);
  double* Z = reinterpret_cast<double*>(base + L.off_z);
  double* PM = reinterpret_cast<double*>(base + L.off_pm);
  double* PS = reinterpret_cast<double*>(base + L.off_ps);
  const int nseg = cv_segments(n, k), DP = cv_dpad(d);

  // the one host-to-device copy of the call: k + 1 offsets (pageable host
  // memory is staged before the call returns)
  ABC_HIP(hipMemcpyAsync(fo, fold_off, sizeof(int64_t) * (k + 1),
                         hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(kde_cv_whiten_kernel,
                     dim3(static_cast<unsigned>(ceil_div(n, 256)), k), dim3(256),
                     0, st, X, w, n, d, DP, mu, Us, Z, NRM, LW2);
  ABC_LAUNCH_CHECK("kde_cv_whiten_kernel");

  const dim3 grid(static_cast<unsigned>(ceil_div(max_nf, kRows)), k, nseg);
#define ABC_CV_G(KS, GN)                                                      \
  case GN:                                                                    \
    hipLaunchKernelGGL((kde_cv_kernel<KS, GN>), grid, dim3(256), 0, st, Z,    \
                       NRM, LW2, n, fo, coef, nseg, PM, PS);                  \
    break;
#define ABC_CV_KS(KS)                                                         \
  switch (G) {                                                                \
    ABC_CV_G(KS, 1) ABC_CV_G(KS, 2) ABC_CV_G(KS, 3) ABC_CV_G(KS, 4)           \
    ABC_CV_G(KS, 5) ABC_CV_G(KS, 6) ABC_CV_G(KS, 7) ABC_CV_G(KS, 8)           \
  }
  if (DP == 4) {
    ABC_CV_KS(1)
  } else if (DP == 8) {
    ABC_CV_KS(2)
  } else if (DP == 16) {
    ABC_CV_KS(4)
  } else {
    ABC_CV_KS(8)
  }
#undef ABC_CV_KS
#undef ABC_CV_G
  ABC_LAUNCH_CHECK("kde_cv_kernel");

  hipLaunchKernelGGL(kde_cv_merge_kernel, dim3(k, G), dim3(256), 0, st, PM, PS,
                     w, n, fo, G, nseg, out_L, out_score);
  ABC_LAUNCH_CHECK("kde_cv_merge_kernel");
  return kOk;
}

}  // extern "C"

namespace abc {
int preload_kde_cv() { return preload_kernel(kde_cv_kernel<2, 5>); }
}  // namespace abc
