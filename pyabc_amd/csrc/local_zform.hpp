// Pieces of the z-form LocalTransition density shared by its two units,
// local_mfma.hip (d <= 8) and local_mfma16.hip (d = 9..16): the grids and
// scales of the f16 piece scheme, the f16 conversions, the per-dimension
// scale, the fragment store and the MFMA wrapper.  Internal linkage.
#pragma once

#include "common.hpp"

namespace abc {

// the d = 9..16 unit (local_mfma16.hip) behind abc_local_logpdf_mfma
size_t lzw_workspace_bytes(int64_t M, int64_t N, int d);
int lzw_run_d(const double* pts, int64_t M, const double* X, const double* w,
              const double* invs, const double* dets, int64_t N, int d, double* out,
              void* ws, hipStream_t st);

namespace {

typedef short h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#ifndef ABC_LZ_WAVES
#define ABC_LZ_WAVES 4
#endif
constexpr int kLzWaves = ABC_LZ_WAVES;  // waves per block sharing the LDS stream
constexpr double kLzGrid = 0.00390625;       // g = 2^-8
constexpr double kLzRowNorm = 7.9;           // |u'| bound of the grid
constexpr float kLzLo = 4096.0f;             // lo pieces x 2^12
constexpr float kLzHalf = 64.0f;             // l2.r2: 2^6 per side
constexpr int kLzTopE = 11;                  // largest column norm -> 2^11
constexpr int kLzMinE = -5;                  // smallest kept: 2^-5 (denormal floor)
constexpr int kLzMaxE = 9;                   // largest unscaled column norm 2^9
constexpr unsigned short kLzOne = 0x3C00;    // f16 1.0
constexpr unsigned short kLzHiPartner = 0x6C00;  // f16 4096.0
// rows whose term sum falls below this take the exact fp64 fixup
constexpr double kLzFixupSum = 2.3283064365386963e-10;  // 2^-32

constexpr int kLzUnitTiles = 8;  // particle tiles per segment unit
constexpr int kLzFlush = 4;      // particle tiles summed in fp32 per fp64 add
constexpr int kLzMaxIB = 4;      // point tiles per wave, largest

__device__ inline unsigned short h16(float x) {  // RNE
  return __builtin_bit_cast(unsigned short, static_cast<_Float16>(x));
}
__device__ inline float h16f(unsigned short b) {
  return static_cast<float>(__builtin_bit_cast(_Float16, b));
}

// largest |X_nb - X_0b| per dimension (ordered keys)
template <int D>
__global__ __launch_bounds__(256) void lz_dims_kernel(const double* __restrict__ X,
                                                      int64_t N,
                                                      unsigned long long* __restrict__ keys) {
  double m[D];
#pragma unroll
  for (int b = 0; b < D; ++b) m[b] = 0.0;
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; n < N;
       n += static_cast<int64_t>(gridDim.x) * 256) {
#pragma unroll
    for (int b = 0; b < D; ++b) m[b] = fmax(m[b], fabs(X[n * D + b] - X[b]));
  }
#pragma unroll
  for (int b = 0; b < D; ++b) {
    block_atomic_max_u64<256>(&keys[b], static_cast<unsigned long long>(f64_key(m[b])));
    __syncthreads();
  }
}

// 2^s_b: the scale putting the population's |x'_b| below 1
__device__ inline double lz_dim_scale(const unsigned long long* keys, int b) {
  const double m = key_f64(keys[b]);
  int E = 0;
  if (m > 0.0) frexp(m, &E);  // m < 2^E
  return ldexp(1.0, -E);
}

// A-operand fragment of row r (of its 32-row tile) for chunk c: slot
// 16 c + 8 hh + e -> F[(tile * KT + c) * 64 + 32 hh + r]
template <int KT>
__device__ inline void lz_store_row(h16x8* __restrict__ F, int64_t tile, int r,
                                    const unsigned short (&v)[16 * KT]) {
#pragma unroll
  for (int c = 0; c < KT; ++c)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      h16x8 x;
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = static_cast<short>(v[16 * c + 8 * hh + e]);
      F[(tile * KT + c) * 64 + 32 * hh + r] = x;
    }
}

__device__ __forceinline__ f32x16 lz_mfma(const h16x8& a, const h16x8& b,
                                          const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a),
                                                __builtin_bit_cast(f16x8, b), c, 0,
                                                0, 0);
}

}  // namespace
}  // namespace abc
