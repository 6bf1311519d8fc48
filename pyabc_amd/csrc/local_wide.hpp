// The exact fp64 LocalTransition density at d = 9..16: its workspace and the
// two host entry points, defined in local.hip, that abc_local_logpdf_f64 and
// local_mfma16.hip (the pass every row takes when a particle flags the
// matrix-core form, and the per-row fixup) both go through -- one copy of
// every kernel, so the two paths give the same bits.
//
// d(d+1)/2 <= 136 packed coefficients per particle do not fit the SGPR file,
// so the d <= 8 form (one thread per point, the particle's coefficients
// wave-uniform through the scalar path) does not carry over.  Here a block
// stages kPdfwBatch particles at a time in LDS as records (X_n | coef_n |
// lc_n - L); every thread reads them at a wave-uniform address (broadcast
// reads, no bank conflicts) and evaluates them against kPdfwPts points of
// its own, which halves the LDS bytes per pair.  The summation contract is
// the d <= 8 one: a fixed number of n-chunks that depends on N only, fp64
// terms under the global offset L = max lc, added in particle order within
// a chunk and in chunk order in the finalize, so a row's bits do not depend
// on M or on the rank count.
#pragma once

#include "local_common.hpp"

namespace abc {

// workspace of the fp64 pass at d > 8: the d <= 8 layout with the
// coefficient block sized by d
struct LocalWsWide {
  double* logsumw;
  unsigned long long* lc_max_key;
  int* n_fix;    // byte 16: the count of fixup rows after the call
  int* n_under;  // byte 20: a second counter, zeroed with it
  double* lc;
  double* coef;
  double* part;
  int* fix_rows;
  int split;
  int64_t nchunk;
};

// Zeroes lc_max_key and n_fix, then log(sum w), lc, max lc and, with
// with_coef, the packed coefficients.
int local_wide_prepare(const double* w, const double* dets, const double* invs,
                       int64_t N, int d, const LocalWsWide& v, bool with_coef,
                       hipStream_t st);
// The fp64 density of a set of rows: all M (rows, count null), or the `count`
// rows listed in `rows` (both on the device; the packed coefficients are then
// built here, when the list holds a row).  Main pass and finalize; the rows
// whose fixed-offset sum underflows are listed in under / n_under and take
// the max-then-sum fixup.  A row's bits do not depend on the set it is in.
void local_wide_pass(const double* pts, int64_t M, const double* X,
                     const double* invs, int64_t N, int d, const LocalWsWide& v,
                     const int* rows, const int* count, int* under, int* n_under,
                     double* out, unsigned fix_grid, hipStream_t st);

namespace {

inline size_t local_ws_wide_bytes(int64_t M, int64_t N, int d) {
  int split;
  int64_t nchunk;
  local_plan(M, N, split, nchunk);
  return 64 + static_cast<size_t>(N) * 8 * (1 + d * (d + 1) / 2) +
         static_cast<size_t>(split) * M * 8 + static_cast<size_t>(M) * 4 + 512;
}

inline LocalWsWide local_ws_wide(void* ws, int64_t M, int64_t N, int d) {
  LocalWsWide v;
  local_plan(M, N, v.split, v.nchunk);
  char* base = static_cast<char*>(ws);
  v.logsumw = reinterpret_cast<double*>(base);
  v.lc_max_key = reinterpret_cast<unsigned long long*>(base + 8);
  v.n_fix = reinterpret_cast<int*>(base + 16);
  v.n_under = reinterpret_cast<int*>(base + 20);
  v.lc = reinterpret_cast<double*>(base + 64);
  v.coef = v.lc + N;
  v.part = v.coef + N * (d * (d + 1) / 2);
  v.fix_rows = reinterpret_cast<int*>(v.part + static_cast<int64_t>(v.split) * M);
  return v;
}

}  // namespace
}  // namespace abc
