// LocalTransition density on the matrix cores at d = 9..16: the z form of
// local_mfma.hip (q_n = |L_n^T (theta - X_n)|^2 as a GEMM of f16 pieces with
// an exact large part, v_mfma_f32_32x32x16_f16) with one particle per lane
// half.
//
// Rows.  A particle takes DP = 16 rows of the 32-row tile (two particles per
// tile, rows d .. 15 zero).  A lane of the 32x32 result holds rows
// 8 k + 4 h + j (k, j < 4) of its half h; component a = 4 k + j of particle p
// sits in row 8 (a >> 2) + 4 p + (a & 3) (lzw_row), so lane half h holds
// particle h whole, component a in accumulator value a.  A (particle, point)
// pair is then d squares in four chains, three adds, one v_exp_f32 and one
// add in the lane, no cross-lane operation; the padding rows cost their
// MFMA share only.
//
// K slots (16 per chunk; KT = KH + KL chunks, a function of d):
//   hi  slot b < d          l1_b               | t1_b 2^12
//       slots d, d + 1      -kappa1 (2 pieces) | 4096
//       -> KH = 1 chunk for d <= 14, 2 for d = 15, 16 (17, 18 slots)
//   lo  slot 16 KH + 5 b + q, q = 0 .. 4:
//       l1_b | r2_b,  l1_b | r3_b,  l2_b 2^12 | t1_b,  l3_b 2^12 | t1_b,
//       l2_b 2^6 | r2_b 2^6
//       slots 16 KH + 5 d, + 1   -kappa_lo 2^12 (2 pieces) | 1
//       -> KL = ceil((5 d + 2) / 16) = 3 (d = 9), 4 (10 - 12), 5 (13 - 15), 6
//   KT = 4, 5, 5, 5, 6, 6, 7, 8 for d = 9 .. 16.
//
// Exactness (DESIGN.md section 4 has the derivation).  With |u'| <= 7.9 on
// the grid g = 2^-8 and the column norm below 2^11 on its grid G_a, the
// rounded vectors satisfy |t1 / g| <= 2022.4 + sqrt(d) / 2 and
// |l1 / G_a| <= 2048 + sqrt(d) / 2, the particle |x1 / g| <= 256 sqrt(d) +
// sqrt(d) / 2.  By Cauchy-Schwarz the absolute sum of the hi products is at
// most 2050 * 2024.4 + 2050 * 1026 = 6.26e6 < 2^23 units of G_a g 2^12 at
// d = 16: every partial sum of the hi chunks, in any order and across the two
// chunks, is an integer below 2^24 and exact in the fp32 accumulator.
// kappa1 / (G_a g) can now reach 2^21.004: its two pieces carry 11 + 11 bits
// (the high one an integer below 2^11 times 2^11), so 2^22 is their limit and
// kLzTopE, the grid and kLzRowNorm stay as at d <= 8.
//
// Fixups and flags are those of d <= 8: a row whose term sum is below 2^-32
// or that lies beyond the grid takes the exact per-row fixup; a particle
// whose Cholesky fails, whose column norms span more than 2^16 or whose
// bandwidth is under the pieces' floor sets the global flag, and then every
// row is a fixup row.  A fixup row goes through the fp64 pass of
// local_wide.hpp restricted to the listed rows: the bits abc_local_logpdf_f64
// gives that row.
//
// Data movement.  Particle fragments stream through LDS by LDS-DMA (TPB
// particle tiles per buffer with their (lc2, cf) pairs, double buffered);
// a wave holds IB 32-point tiles in registers (IB KT 4 VGPRs) and two
// accumulators in flight; the VALU stages of one product run in the MFMA
// gaps of the next.  Segments depend on N only; fp32 over kLzFlush particle
// tiles, then fp64 in fixed order: a row's bits do not depend on M, IB, TPB
// or the number of ranks.
#include <cmath>

#include "common.hpp"
#include "local_common.hpp"
#include "local_wide.hpp"
#include "local_zform.hpp"

namespace abc {
namespace {

template <int D>
struct Lzw {
  static_assert(D >= 9 && D <= 16, "the wide z form serves d = 9..16");
  static constexpr int DP = 16;                     // rows per particle
  static constexpr int PT = 2;                      // particles per 32-row tile
  static constexpr int KH = (D + 2 + 15) / 16;      // hi chunks
  static constexpr int KL = (5 * D + 2 + 15) / 16;  // lo chunks
  static constexpr int KT = KH + KL;
  static constexpr int LO = 16 * KH;                // first lo slot
  // point tiles per wave and particle tiles per LDS buffer, from the code
  // objects: two waves per SIMD and no spill; the
  // static LDS limit (64 KiB) holds TPB = 4 up to KT = 7
  static constexpr int IB = KT <= 6 ? 4 : 2;
  static constexpr int TPB = KT <= 7 ? 4 : 2;
};

// row of component a of tile particle p: lane half p holds it as value a
__device__ __forceinline__ int lzw_row(int p, int a) {
  return 8 * (a >> 2) + 4 * p + (a & 3);
}

// One thread per particle: Cholesky of inv_n (in scratch: a prep kernel),
// then per component the scaled column, its pieces and the kappa constants
// -> 16 rows of A fragments; (lc2, cf) in particle order
template <int D>
__global__ __launch_bounds__(128) void lzw_pack_prev_kernel(
    const double* __restrict__ X, const double* __restrict__ invs,
    const double* __restrict__ lc, const unsigned long long* __restrict__ lc_max_key,
    int64_t N, int64_t npad, const unsigned long long* __restrict__ dkeys,
    h16x8* __restrict__ A, float2* __restrict__ lcT, int* __restrict__ gflag) {
  using P = Lzw<D>;
  constexpr int KT = P::KT, LO = P::LO;
  const int64_t n = static_cast<int64_t>(blockIdx.x) * 128 + threadIdx.x;
  if (n >= npad) return;
  const int64_t tile = n / P::PT;
  const int pin = static_cast<int>(n % P::PT);
  bool ok = n < N;
  double L[D][D], sc[D], xs[D], x1[D];
  int ea[D];
  int F = 0;
  const double c = 0.84932180028801907;  // sqrt(log2(e) / 2)
  if (ok) {
#pragma unroll
    for (int b = 0; b < D; ++b) {
      sc[b] = lz_dim_scale(dkeys, b);
      xs[b] = (X[n * D + b] - X[b]) * sc[b];
      x1[b] = rint(xs[b] / kLzGrid) * kLzGrid;
    }
    // Cholesky P = L L^T (row-major symmetric inv_n)
    const double* Pn = invs + n * D * D;
#pragma unroll 1
    for (int j = 0; j < D; ++j) {
      double s = Pn[j * D + j];
      for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
      ok = ok && s > 0.0;
      const double djj = s > 0.0 ? sqrt(s) : 1.0;
      L[j][j] = djj;
#pragma unroll 1
      for (int i = j + 1; i < D; ++i) {
        double t = 0.5 * (Pn[i * D + j] + Pn[j * D + i]);
        for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
        L[i][j] = t / djj;
      }
    }
    // norms of the scaled columns lhat_ba = L_ba 2^-s_b sqrt(log2 e / 2)
    int emax = -1000, emin = 1000;
#pragma unroll 1
    for (int a = 0; a < D; ++a) {
      double nn = 0.0;
      for (int b = a; b < D; ++b) {
        const double lh = L[b][a] / sc[b] * c;
        nn = fma(lh, lh, nn);
      }
      int E = 0;
      frexp(sqrt(nn), &E);  // |l| < 2^E
      ea[a] = nn > 0.0 ? E : -1000;
      if (nn > 0.0) {
        emax = ea[a] > emax ? ea[a] : emax;
        emin = ea[a] < emin ? ea[a] : emin;
      }
      ok = ok && nn > 0.0 && nn == nn;
    }
    // the precision floor and the f16 range of the pieces (local_mfma.hip)
    ok = ok && emax <= kLzMaxE;
    F = kLzTopE - emax;
    ok = ok && emin + F >= kLzMinE;
    if (!ok) atomicOr(gflag, 1);
  }
#pragma unroll 1
  for (int a = 0; a < P::DP; ++a) {
    unsigned short v[16 * KT];
#pragma unroll
    for (int k = 0; k < 16 * KT; ++k) v[k] = 0;
    if (ok && a < D) {
      const double G = ldexp(1.0, ea[a] + F - kLzTopE);
      double k1 = 0.0, klo = 0.0;
#pragma unroll
      for (int b = 0; b < D; ++b) {
        const double l = ldexp(b >= a ? L[b][a] / sc[b] * c : 0.0, F);
        const double l1 = rint(l / G) * G;
        const unsigned short p2 = h16(static_cast<float>((l - l1) * kLzLo));
        const double l2 = static_cast<double>(h16f(p2)) / kLzLo;
        const unsigned short p3 = h16(static_cast<float>((l - l1 - l2) * kLzLo));
        const double l3 = static_cast<double>(h16f(p3)) / kLzLo;
        v[b] = h16(static_cast<float>(l1));  // hi: l1 | t1 2^12
        v[LO + 5 * b + 0] = v[b];            // l1 | r2
        v[LO + 5 * b + 1] = v[b];            // l1 | r3
        v[LO + 5 * b + 2] = p2;              // l2 2^12 | t1
        v[LO + 5 * b + 3] = p3;              // l3 2^12 | t1
        v[LO + 5 * b + 4] = h16(static_cast<float>(l2 * kLzHalf));  // l2 2^6 | r2 2^6
        k1 = fma(l1, x1[b], k1);             // exact (multiples of G g)
        klo += l1 * (xs[b] - x1[b]) + (l2 + l3) * xs[b];
      }
      // -kappa1 in two f16 pieces (K = kappa1 / (G g) < 2^22: 11 + 11 bits)
      const double Gg = G * kLzGrid;
      const double K = rint(k1 / Gg);
      const double K0 = trunc(K / 2048.0) * 2048.0;
      v[D] = h16(static_cast<float>(-K0 * Gg));
      v[D + 1] = h16(static_cast<float>(-(K - K0) * Gg));
      // -kappa_lo x 2^12 in two pieces
      const double kl = -klo * kLzLo;
      const unsigned short q0 = h16(static_cast<float>(kl));
      v[LO + 5 * D] = q0;
      v[LO + 5 * D + 1] = h16(static_cast<float>(kl - static_cast<double>(h16f(q0))));
    }
    lz_store_row<KT>(A, tile, lzw_row(pin, a), v);
  }
  float2 lcv = make_float2(-INFINITY, 0.0f);
  if (ok)
    lcv = make_float2(
        static_cast<float>((lc[n] - key_f64(*lc_max_key)) * 1.4426950408889634),
        -ldexpf(1.0f, -24 - 2 * F));
  lcT[n] = lcv;
}

// One thread per evaluation point: its pieces in B-operand order
template <int D>
__global__ __launch_bounds__(256) void lzw_pack_new_kernel(
    const double* __restrict__ pts, int64_t M, int64_t mpad,
    const double* __restrict__ X, const unsigned long long* __restrict__ dkeys,
    h16x8* __restrict__ B, int* __restrict__ rflag) {
  constexpr int KT = Lzw<D>::KT, LO = Lzw<D>::LO;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= mpad) return;
  unsigned short v[16 * KT];
#pragma unroll
  for (int k = 0; k < 16 * KT; ++k) v[k] = 0;
  bool ok = i < M;
  double us[D];
  if (ok) {
    double nn = 0.0;
#pragma unroll
    for (int b = 0; b < D; ++b) {
      us[b] = (pts[i * D + b] - X[b]) * lz_dim_scale(dkeys, b);
      nn = fma(us[b], us[b], nn);
    }
    ok = sqrt(nn) <= kLzRowNorm;  // NaN -> false
  }
  if (ok) {
#pragma unroll
    for (int b = 0; b < D; ++b) {
      const double t1 = rint(us[b] / kLzGrid) * kLzGrid;
      const double r = us[b] - t1;
      const unsigned short r2 = h16(static_cast<float>(r * kLzLo));
      const double r2v = static_cast<double>(h16f(r2)) / kLzLo;
      const unsigned short r3 = h16(static_cast<float>((r - r2v) * kLzLo));
      const unsigned short t1b = h16(static_cast<float>(t1));
      v[b] = h16(static_cast<float>(t1 * kLzLo));  // exact: |t1| < 8
      v[LO + 5 * b + 0] = r2;
      v[LO + 5 * b + 1] = r3;
      v[LO + 5 * b + 2] = t1b;
      v[LO + 5 * b + 3] = t1b;
      v[LO + 5 * b + 4] = h16(static_cast<float>(r2v * kLzHalf));
    }
    v[D] = v[D + 1] = kLzHiPartner;
    v[LO + 5 * D] = v[LO + 5 * D + 1] = kLzOne;
  }
  if (i < M) rflag[i] = ok ? 0 : 1;
  lz_store_row<KT>(B, i >> 5, static_cast<int>(i & 31), v);
}

// The squares of one (particle, point) pair in two stages of two chains of
// four components each (stage G: components 8 G ..), only the D real ones;
// q = (c0 + c1) + (c2 + c3).
template <int D, int G>
__device__ __forceinline__ void lzw_squares(const f32x16& acc, float (&q)[2]) {
  constexpr int B0 = 8 * G;
  float x = acc[B0] * acc[B0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (B0 + j < D) x = __builtin_fmaf(acc[B0 + j], acc[B0 + j], x);
  if constexpr (B0 + 4 < D) {
    float y = acc[B0 + 4] * acc[B0 + 4];
#pragma unroll
    for (int j = 5; j < 8; ++j)
      if (B0 + j < D) y = __builtin_fmaf(acc[B0 + j], acc[B0 + j], y);
    x += y;
  }
  q[G] = x;
}

// Block (segment s, row block rb), segment major; wave w owns point tiles
// (rb * kLzWaves + w) * IB ...  Per segment one fp64 partial per point; the
// fp32 terms are flushed into it every kLzFlush particle tiles whatever TPB
// and IB, so a row's bits do not depend on either.
template <int D, int IB, int TPB>
__global__ __launch_bounds__(64 * kLzWaves) void lzw_kernel(
    const h16x8* __restrict__ Bfr, int64_t M, const h16x8* __restrict__ Afr,
    const float2* __restrict__ lcT, int64_t npad, int nseg, int64_t seg_len,
    const int* __restrict__ gflag, double* __restrict__ part) {
  using P = Lzw<D>;
  constexpr int KT = P::KT, PT = P::PT;
  constexpr int CH = TPB * KT;  // fragments per LDS buffer
  static_assert(kLzUnitTiles % TPB == 0 && kLzFlush % TPB == 0, "TPB: 1, 2 or 4");
  __shared__ h16x8 As[2][CH][64];
  // (lc2, cf) of the buffer's TPB PT particles (the first 2 TPB PT floats),
  // DMA'd with it one dword per lane
  __shared__ float Lc[2][64];
  if (*gflag) return;  // every row takes the exact fp64 pass
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nrb = gridDim.x / nseg;
  const int s = static_cast<int>(blockIdx.x / nrb);
  const int64_t rb = blockIdx.x % nrb;
  const int64_t t0 = (rb * kLzWaves + wave) * IB;
  const int h = lane >> 5;
  h16x8 bq[IB][KT];
#pragma unroll
  for (int t = 0; t < IB; ++t)
#pragma unroll
    for (int c = 0; c < KT; ++c) bq[t][c] = Bfr[((t0 + t) * KT + c) * 64 + lane];
  const int64_t p0 = static_cast<int64_t>(s) * seg_len;
  int64_t p1 = p0 + seg_len;
  if (p1 > npad) p1 = npad;
  const int64_t tile0 = p0 / PT, ntile = (p1 - p0) / PT;  // a multiple of 8
  const h16x8* __restrict__ Aseg = Afr + tile0 * KT * 64;
  const float* __restrict__ Lseg = reinterpret_cast<const float*>(lcT + tile0 * PT);
  auto fill = [&](int buf, int64_t tl) {
    const h16x8* __restrict__ src = Aseg + tl * KT * 64;
    for (int f = wave; f < CH; f += kLzWaves)
      __builtin_amdgcn_global_load_lds(
          src + f * 64 + lane, (__attribute__((address_space(3))) void*)&As[buf][f][0],
          16, 0, 0);
    // lcT carries 512 bytes of slack behind the last particle
    if (wave == kLzWaves - 1)
      __builtin_amdgcn_global_load_lds(
          Lseg + tl * PT * 2 + lane,
          (__attribute__((address_space(3))) void*)&Lc[buf][0], 4, 0, 0);
  };
  double S[IB];
  float sacc[IB];
#pragma unroll
  for (int t = 0; t < IB; ++t) S[t] = 0.0;
  if (ntile > 0) fill(0, 0);
  int buf = 0;
  for (int64_t tl = 0; tl < ntile; tl += TPB) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tl + TPB < ntile) fill(buf ^ 1, tl + TPB);
    const float2* __restrict__ Lb = reinterpret_cast<const float2*>(&Lc[buf][0]);
    // A fragments of particle tile u, read one product before their first
    // MFMA (a ring of two)
    h16x8 a[2][KT];
#pragma unroll
    for (int c = 0; c < KT; ++c) a[0][c] = As[buf][c][lane];
    // the TPB IB products of this buffer, software pipelined as in lz_kernel:
    // stage st of product p runs in MFMA gap KT (p + 1) + 1 + st, from the
    // second MFMA of product p + 1 on -- its accumulator has landed by then;
    // KT >= 4, so the stages end inside product p + 1 and two accumulators
    // alternate
    constexpr int NQ = TPB * IB;
    static_assert(KT >= 4, "the three stages of a product fit the next one's gaps");
    f32x16 acc[2];
    float qv[2][2];
#pragma unroll
    for (int q = 0; q < NQ + 1; ++q) {
      if (q < NQ) acc[q % 2] = f32x16{};
#pragma unroll
      for (int c = 0; c < KT; ++c) {
        if (q < NQ) acc[q % 2] = lz_mfma(a[(q / IB) & 1][c], bq[q % IB][c], acc[q % 2]);
        __builtin_amdgcn_sched_barrier(0);
        // the next particle tile's fragments, one product ahead
        if (c == 0 && q % IB == IB - 1 && q / IB + 1 < TPB) {
          const int un = q / IB + 1;
#pragma unroll
          for (int cc = 0; cc < KT; ++cc) a[un & 1][cc] = As[buf][un * KT + cc][lane];
        }
        // the stages due in this gap, older products first
#pragma unroll
        for (int st = 2; st >= 0; --st) {
          const int pos = KT * q + c - 1 - st;  // = KT (p + 1) for stage st of p
          if (pos < 0 || pos % KT != 0) continue;
          const int p = pos / KT - 1;
          if (p < 0 || p >= NQ) continue;
          const int u = p / IB, t = p % IB;
          if (st == 0) {
            // the accumulator stays allocated whole until here (its padding
            // values are not reused while the MFMA writing them is in flight)
            asm volatile("" ::"v"(acc[p % 2]));
            lzw_squares<D, 0>(acc[p % 2], qv[p & 1]);
          }
          if (st == 1) lzw_squares<D, 1>(acc[p % 2], qv[p & 1]);
          if (st == 2) {
            const float2 lcv = Lb[u * PT + h];
            const float v = __builtin_amdgcn_exp2f(
                __builtin_fmaf(qv[p & 1][0] + qv[p & 1][1], lcv.y, lcv.x));
            // fp32 over kLzFlush consecutive particle tiles, then into fp64
            const int tg = TPB == kLzFlush ? u : static_cast<int>((tl + u) % kLzFlush);
            sacc[t] = tg == 0 ? v : sacc[t] + v;
            if (tg == kLzFlush - 1) S[t] += static_cast<double>(sacc[t]);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    buf ^= 1;
  }
#pragma unroll
  for (int t = 0; t < IB; ++t) {
    const double tot = S[t] + __shfl_xor(S[t], 32, 64);
    const int64_t i = (t0 + t) * 32 + lane;
    if (lane < 32 && i < M) part[static_cast<int64_t>(s) * M + i] = tot;
  }
}

// Rows of the matrix-core pass: the log density, or the fixup list -- every
// row with the flag set.
__global__ __launch_bounds__(256) void lzw_final_kernel(
    const double* __restrict__ part, int64_t M, int nseg,
    const unsigned long long* __restrict__ lc_max_key,
    const double* __restrict__ logsumw, const int* __restrict__ gflag,
    const int* __restrict__ rflag, double* __restrict__ out,
    int* __restrict__ n_fix, int* __restrict__ fix_rows) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= M) return;
  double S = 0.0;
  if (!*gflag)
    for (int s = 0; s < nseg; ++s) S += part[s * M + i];
  if (!*gflag && !rflag[i] && S >= kLzFixupSum) {
    out[i] = key_f64(*lc_max_key) + log(S) - *logsumw;
  } else {
    fix_rows[atomicAdd(n_fix, 1)] = static_cast<int>(i);
    out[i] = -INFINITY;
  }
}

struct LzwPlan {
  int64_t npad, mpad, seg_len;
  int nseg;
  size_t a_bytes, b_bytes, lc_bytes;
};

template <int D>
LzwPlan lzw_plan(int64_t M, int64_t N) {
  using P = Lzw<D>;
  LzwPlan p;
  int split;
  int64_t nchunk;
  local_plan(M, N, split, nchunk);
  const int64_t unit = kLzUnitTiles * P::PT;  // 16 particles
  p.seg_len = ceil_div(nchunk, unit) * unit;
  p.npad = ceil_div(N, unit) * unit;
  p.nseg = static_cast<int>(ceil_div(p.npad, p.seg_len));  // <= split
  const int64_t rows = 32 * kLzWaves * kLzMaxIB;  // every IB divides it
  p.mpad = ceil_div(M, rows) * rows;
  p.a_bytes = static_cast<size_t>(p.npad / P::PT) * P::KT * 64 * 16;
  p.b_bytes = static_cast<size_t>(p.mpad / 32) * P::KT * 64 * 16;
  p.lc_bytes = static_cast<size_t>(p.npad) * 8 + 512;  // + the DMA's slack
  return p;
}

inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// behind the fp64 pass's workspace: dims keys (128) + flag | rflag[M] | lcT
// | A | B, 256-aligned pieces
template <int D>
size_t lzw_bytes(int64_t M, int64_t N) {
  const LzwPlan p = lzw_plan<D>(M, N);
  return up256(local_ws_wide_bytes(M, N, D)) + 256 + up256(static_cast<size_t>(M) * 4) +
         up256(p.lc_bytes) + up256(p.a_bytes) + up256(p.b_bytes);
}

template <int D>
int lzw_run(const double* pts, int64_t M, const double* X, const double* w,
            const double* invs, const double* dets, int64_t N, double* out,
            void* ws, hipStream_t st) {
  const LzwPlan p = lzw_plan<D>(M, N);
  const LocalWsWide v = local_ws_wide(ws, M, N, D);
  char* base = static_cast<char*>(ws);
  char* ex = base + up256(local_ws_wide_bytes(M, N, D));
  unsigned long long* dkeys = reinterpret_cast<unsigned long long*>(ex);
  int* gflag = reinterpret_cast<int*>(ex + 128);
  int* rflag = reinterpret_cast<int*>(ex + 256);
  char* q = ex + 256 + up256(static_cast<size_t>(M) * 4);
  float2* lcT = reinterpret_cast<float2*>(q);
  q += up256(p.lc_bytes);
  h16x8* A = reinterpret_cast<h16x8*>(q);
  q += up256(p.a_bytes);
  h16x8* B = reinterpret_cast<h16x8*>(q);
  ABC_HIP(hipMemsetAsync(ex, 0, 256, st));
  // the packed coefficients only for fixup rows or the flag (local_wide_pass)
  const int rc = local_wide_prepare(w, dets, invs, N, D, v, false, st);
  if (rc != kOk) return rc;
  hipLaunchKernelGGL(lz_dims_kernel<D>, dim3(stream_grid(N, 256, 512)), dim3(256),
                     0, st, X, N, dkeys);
  hipLaunchKernelGGL(lzw_pack_prev_kernel<D>, dim3(ceil_div(p.npad, 128)), dim3(128),
                     0, st, X, invs, v.lc, v.lc_max_key, N, p.npad, dkeys, A, lcT, gflag);
  hipLaunchKernelGGL(lzw_pack_new_kernel<D>, dim3(ceil_div(p.mpad, 256)), dim3(256),
                     0, st, pts, M, p.mpad, X, dkeys, B, rflag);
  // launch-shape knobs (rows bit-identical): values the unit has no kernel
  // for keep the default
  int ib = Lzw<D>::IB, tpb = Lzw<D>::TPB;
  {
    const int k = tuning_knob(kKnobLzIb, ib);
    if (k == 1 || k == 2 || (k == 4 && Lzw<D>::IB == 4)) ib = k;
  }
  {
    const int k = tuning_knob(kKnobLzTpb, tpb);
    if (k == 2 || (k == 4 && Lzw<D>::TPB == 4)) tpb = k;
  }
  const unsigned grid =
      static_cast<unsigned>(p.mpad / (32 * kLzWaves * ib) * p.nseg);
#define LZW_LAUNCH(IBV, TPBV)                                                      \
  hipLaunchKernelGGL((lzw_kernel<D, IBV, TPBV>), dim3(grid), dim3(64 * kLzWaves), 0, \
                     st, B, M, A, lcT, p.npad, p.nseg, p.seg_len, gflag, v.part)
#define LZW_IB(TPBV)                                               \
  do {                                                             \
    if constexpr (Lzw<D>::IB == 4) {                               \
      if (ib == 4) LZW_LAUNCH(4, TPBV);                            \
    }                                                              \
    if (ib == 2) LZW_LAUNCH(2, TPBV);                              \
    if (ib == 1) LZW_LAUNCH(1, TPBV);                              \
  } while (0)
  if constexpr (Lzw<D>::TPB == 4) {
    if (tpb == 4) LZW_IB(4);
  }
  if (tpb == 2) LZW_IB(2);
#undef LZW_IB
#undef LZW_LAUNCH
  hipLaunchKernelGGL(lzw_final_kernel, dim3(ceil_div(M, 256)), dim3(256), 0, st, v.part,
                     M, p.nseg, v.lc_max_key, v.logsumw, gflag, rflag, out, v.n_fix,
                     v.fix_rows);
  // the listed rows through the fp64 pass (rflag is free: it takes the list
  // of the rows that underflow there too)
  local_wide_pass(pts, M, X, invs, N, D, v, v.fix_rows, v.n_fix, rflag, v.n_under, out,
                  1024, st);
  return kOk;
}

}  // namespace

size_t lzw_workspace_bytes(int64_t M, int64_t N, int d) {
  switch (d) {
#define C(DD) \
  case DD: return lzw_bytes<DD>(M, N);
    C(9) C(10) C(11) C(12) C(13) C(14) C(15) C(16)
#undef C
  }
  return 0;
}

int lzw_run_d(const double* pts, int64_t M, const double* X, const double* w,
              const double* invs, const double* dets, int64_t N, int d, double* out,
              void* ws, hipStream_t st) {
  switch (d) {
#define C(DD) \
  case DD: return lzw_run<DD>(pts, M, X, w, invs, dets, N, out, ws, st);
    C(9) C(10) C(11) C(12) C(13) C(14) C(15) C(16)
#undef C
  }
  set_error("local_logpdf_mfma: unsupported d=%d", d);
  return kUnsupported;
}

// Loads this unit's code object (abc_preload calls every unit's hook).
int preload_local_mfma16() { return preload_kernel(lzw_final_kernel); }

}  // namespace abc
