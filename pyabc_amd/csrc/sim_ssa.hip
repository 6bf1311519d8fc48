// Mass-action reaction-network Markov jump process (MassActionSSAModel): the
// stochastic half of the reference's worked examples
// (doc/examples/chemical_reaction.ipynb), where the model is Gillespie's
// direct method in a Python loop per proposal.  Same network table as the ODE
// model (sim_ode.hip), integer molecule counts, one lane per proposal:
//
//   a_r = k_r * x_a * x_b   (empty slot: 1; second slot of 2A: x_A - 1)
//   a0  = a_0 + ... + a_{R-1}, summed in order, afresh every event
//   tau = -log(1 - u1) / a0,  fire the first r with a_0 + ... + a_r > u2 * a0
//   (u1, u2) = the two 53-bit uniforms of Philox block (g << 24) | e
//
// Every add and multiply of this arithmetic is rounded on its own (fp
// contraction is off for the whole unit), so a host replay that sums in the
// same order picks the same reaction (include/abc_hip.h states the process).
//
// Where the data lives ("Mass-action SSA model"):
//   * the network table and the 16 dependency masks are kernel arguments BY
//     VALUE, read through wave-uniform indices: scalar loads, scalar
//     compares.  The one per-lane index into the table is the observation
//     counter j (t_obs[j]): a vector load from the argument segment, once per
//     observation crossed, never per event;
//   * the counts are int32 in VGPRs, unrolled over the template parameter N;
//     a wave-uniform species index is resolved by a select chain;
//   * per-lane rates k_r and propensities a_r sit in LDS, [r][lane] and
//     [R + r][lane]: the arrays whose index is a run-time value.  A lane reads
//     only what it wrote: no barrier;
//   * the reaction a lane fires is a per-lane value.  It is applied by a
//     wave-uniform loop over the reactions with the lanes that fired r
//     enabled, so the stoichiometry stays a scalar read; the same loop hands
//     the lane the mask of propensities to recompute.
// No matrix instructions: a state per lane, an event time per lane and a
// sparse stoichiometry leave no dense tile to feed them.
//
// Two forms, the same bits (a column depends on theta row, seed, sid and g
// only): ssa_plain_kernel gives a wave 64 consecutive proposals and retires
// it with its slowest lane; ssa_refill_kernel is a persistent grid whose idle
// lanes claim the next proposals from a device counter, one wave-aggregated
// atomic per refill round.
#include <atomic>

#include "common.hpp"
#include "philox.hpp"
#include "../../include/abc_hip.h"

#pragma clang fp contract(off)

namespace abc {

constexpr int kSsaBlock = 64;       // one wave; nothing is shared between lanes
constexpr int kSsaRefillMin = 16;   // idle lanes before a wave claims work
constexpr int kSsaWavesPerCu = 16;  // persistent grid: four waves per SIMD
constexpr int kSsaSlots = 64;       // claim counters: calls in flight per device
constexpr int64_t kSsaMaxEvents = int64_t{1} << 24;

// dependency masks: bit q of m[r] = reaction q has a reactant whose count
// reaction r changes
struct SsaDeps {
  uint16_t m[ABC_ODE_MAX_REACTIONS];
};

__device__ unsigned long long g_ssa_next[kSsaSlots];

// what the kernels share beyond the table
struct SsaArgs {
  const double* theta;
  double* out_T;
  int64_t* events_out;
  int64_t B, ld, max_events;
  uint64_t seed, sid, offset;
  int d;
};

template <int N>
struct SsaLane {
  int32_t x[N];
  double t, tj;  // time of the last event, next observation time
  int64_t b;
  int j, e;      // observations stored, events fired
};

// x[i] for a wave-uniform i in [0, N)
template <int N>
__device__ __forceinline__ int32_t pick(const int32_t (&x)[N], int i) {
  int32_t r = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) r = i == k ? x[k] : r;
  return r;
}

// (k * x_a) * x_b, the second factor of 2A being x_A - 1
template <int N>
__device__ __forceinline__ double propensity(const abc_ode_table& T, int r,
                                             double k, const int32_t (&x)[N]) {
  const int a = T.reactant[r][0], c = T.reactant[r][1];
  if (a >= 0) k *= static_cast<double>(pick<N>(x, a));
  if (c >= 0) k *= static_cast<double>(pick<N>(x, c) - (c == a ? 1 : 0));
  return k;
}

template <int N>
__device__ __forceinline__ void store_obs(const abc_ode_table& T, const SsaArgs& A,
                                          const SsaLane<N>& L, int j) {
  int o = 0;
#pragma unroll 1
  do {
    A.out_T[static_cast<int64_t>(o * T.n_times + j) * A.ld + L.b] =
        static_cast<double>(pick<N>(L.x, T.observed[o]));
  } while (++o < T.n_observed);
}

template <int N>
__device__ __forceinline__ void store_failed(const abc_ode_table& T, const SsaArgs& A,
                                             const SsaLane<N>& L) {
  const int S = T.n_times * T.n_observed;
  int s = 0;
#pragma unroll 1
  do {
    A.out_T[static_cast<int64_t>(s) * A.ld + L.b] = INFINITY;
  } while (++s < S);
  if (A.events_out) A.events_out[L.b] = L.e;
}

// start proposal b in this lane; false when it fails at once
template <int N>
__device__ __forceinline__ bool ssa_init(const abc_ode_table& T, const SsaArgs& A,
                                         double* lds, int64_t b, SsaLane<N>& L) {
  const double* th = A.theta + b * A.d;
  const int R = T.n_reactions;
  bool ok = true;
  int r = 0;
#pragma unroll 1
  do {
    const int kind = T.rate_kind[r];
    double k = T.rate_const[r];
    if (kind != 0) {
      k = th[T.rate_col[r]];
      if (kind == 2) k = exp10(k);
    }
    ok = ok && k >= 0.0 && k < INFINITY;
    lds[r * kSsaBlock] = k;
  } while (++r < R);
  // a rolled loop with a scatter, so that the table's initial values are
  // read when a proposal starts and not held in scalar registers meanwhile
#pragma unroll
  for (int k = 0; k < N; ++k) L.x[k] = 0;
  int i = 0;
#pragma unroll 1
  do {
    const int col = T.x_init_col[i];
    double v = T.x_init[i];  // a checked integer in [0, 2^31)
    if (col >= 0) {
      v = rint(th[col]);
      ok = ok && v >= 0.0 && v < 2147483648.0;
    }
    const int32_t xi = ok ? static_cast<int32_t>(v) : 0;
#pragma unroll
    for (int k = 0; k < N; ++k) L.x[k] = i == k ? xi : L.x[k];
  } while (++i < N);
  r = 0;
#pragma unroll 1
  do {
    lds[(R + r) * kSsaBlock] = propensity<N>(T, r, lds[r * kSsaBlock], L.x);
  } while (++r < R);
  L.t = 0.0;
  L.tj = T.t_obs[0];
  L.b = b;
  L.j = 0;
  L.e = 0;
  if (!ok) store_failed<N>(T, A, L);
  return ok;
}

// one event of the lane's proposal; false when the proposal has ended
template <int N>
__device__ __forceinline__ bool ssa_event(const abc_ode_table& T, const SsaDeps& D,
                                          const SsaArgs& A, double* lds,
                                          SsaLane<N>& L) {
  const int R = T.n_reactions, n_times = T.n_times;
  const double* al = lds + R * kSsaBlock;
  double a0 = 0.0;
  int r = 0;
#pragma unroll 1
  do a0 += al[r * kSsaBlock];
  while (++r < R);
  double tn = INFINITY;  // a0 == 0: nothing fires again
  double target = 0.0;
  if (a0 != 0.0) {
    const uint64_t g = A.offset + static_cast<uint64_t>(L.b);
    // the key is re-read here every event: its ten-round schedule is scalar
    // adds, cheaper than twenty scalar registers held across the loop
    uint32_t k0 = static_cast<uint32_t>(A.seed), k1 = static_cast<uint32_t>(A.seed >> 32);
    asm volatile("" : "+s"(k0), "+s"(k1));
    const uint64_t ctr = (g << 24) | static_cast<uint64_t>(L.e);
    const u32x4 w = philox4x32_10(
        u32x4{static_cast<uint32_t>(ctr), static_cast<uint32_t>(ctr >> 32),
              static_cast<uint32_t>(A.sid), static_cast<uint32_t>(A.sid >> 32)}, k0, k1);
    tn = L.t + -log(1.0 - u53(w.x, w.y)) / a0;
    target = u53(w.z, w.w) * a0;
  }
  while (L.j < n_times && L.tj < tn) {
    store_obs<N>(T, A, L, L.j);
    ++L.j;
    if (L.j < n_times) L.tj = T.t_obs[L.j];
  }
  if (L.j == n_times) {
    if (A.events_out) A.events_out[L.b] = L.e;
    return false;
  }
  int fired = -1, last = 0;
  double s = 0.0;
  r = 0;
#pragma unroll 1
  do {
    const double ar = al[r * kSsaBlock];
    s += ar;
    fired = (fired < 0 && s > target) ? r : fired;
    last = ar > 0.0 ? r : last;
  } while (++r < R);
  fired = fired < 0 ? last : fired;
  // the lanes that fired r apply its net stoichiometry and take its mask
  unsigned mask = 0;
  bool ok = true;
  r = 0;
#pragma unroll 1
  do {
    if (fired != r) continue;
    mask = D.m[r];
    const int p1 = T.pair_start[r + 1];
#pragma unroll 1
    for (int p = T.pair_start[r]; p < p1; ++p) {
      const int pe = T.pair[p];
      const int sp = pe & 0xff, nu = pe >> 8;
#pragma unroll
      for (int i = 0; i < N; ++i)
        if (sp == i) {
          const int64_t v = static_cast<int64_t>(L.x[i]) + nu;
          ok = ok && v >= 0 && v <= 0x7fffffff;
          L.x[i] = static_cast<int32_t>(v);
        }
    }
  } while (++r < R);
  r = 0;
#pragma unroll 1
  do {
    if ((mask >> r) & 1u)
      lds[(R + r) * kSsaBlock] = propensity<N>(T, r, lds[r * kSsaBlock], L.x);
  } while (++r < R);
  L.t = tn;
  ++L.e;
  if (!ok || L.e >= A.max_events) {
    store_failed<N>(T, A, L);
    return false;
  }
  return true;
}

// the loop runs at most max_events + 1 times: every pass fires or ends
template <int N>
__global__ __launch_bounds__(kSsaBlock) void ssa_plain_kernel(
    const abc_ode_table T, const SsaDeps D, const SsaArgs A) {
  extern __shared__ double ssa_lds[];  // [2 R][kSsaBlock]
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kSsaBlock + threadIdx.x;
  if (b >= A.B) return;
  double* lds = ssa_lds + threadIdx.x;
  SsaLane<N> L;
  bool active = ssa_init<N>(T, A, lds, b, L);
  while (active) active = ssa_event<N>(T, D, A, lds, L);
}

// Every pass either fires an event in some lane, ends a proposal or claims
// from the counter, which only grows and ends the wave once it has passed B:
// at most B (max_events + 2) passes, and no wave waits for another.
template <int N>
__global__ __launch_bounds__(kSsaBlock) void ssa_refill_kernel(
    const abc_ode_table T, const SsaDeps D, const SsaArgs A, int slot) {
  extern __shared__ double ssa_lds[];
  double* lds = ssa_lds + threadIdx.x;
  SsaLane<N> L;
  bool active = false, drained = false;
  for (;;) {
    const unsigned long long idle = __ballot(!active);
    const int n_idle = __popcll(idle);
    if (!drained && n_idle >= kSsaRefillMin) {
      const int first = __ffsll(idle) - 1;
      unsigned long long base = 0;
      if (static_cast<int>(threadIdx.x) == first)
        base = atomicAdd(&g_ssa_next[slot], static_cast<unsigned long long>(n_idle));
      base = __shfl(base, first, kSsaBlock);
      drained = base + n_idle >= static_cast<unsigned long long>(A.B);
      if (!active) {
        const unsigned lo = static_cast<unsigned>(idle), hi = static_cast<unsigned>(idle >> 32);
        const unsigned rank = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
        const unsigned long long b = base + rank;
        if (b < static_cast<unsigned long long>(A.B))
          active = ssa_init<N>(T, A, lds, static_cast<int64_t>(b), L);
      }
    }
    if (__ballot(active) == 0) {
      if (drained) break;
      continue;  // every claimed proposal failed at once: claim again
    }
    if (active) active = ssa_event<N>(T, D, A, lds, L);
  }
}

__global__ void ssa_zero_kernel(int slot) { g_ssa_next[slot] = 0; }

}  // namespace abc

using namespace abc;

extern "C" {

int abc_sim_mass_action_ssa_f64(const abc_ode_table* table, const double* theta,
                                int64_t B, int d, int64_t max_events, uint64_t seed,
                                uint64_t sid, uint64_t offset, double* out_T,
                                int64_t ld, int64_t* events_out, hipStream_t st) {
  ABC_REQUIRE(table, "sim_mass_action_ssa: null table");
  const abc_ode_table& T = *table;
  const int n = T.n_species, R = T.n_reactions;
  ABC_REQUIRE(n >= 1 && n <= ABC_ODE_MAX_SPECIES,
              "sim_mass_action_ssa: 1 <= n_species <= 8");
  ABC_REQUIRE(R >= 1 && R <= ABC_ODE_MAX_REACTIONS,
              "sim_mass_action_ssa: 1 <= n_reactions <= 16");
  ABC_REQUIRE(T.n_times >= 1 && T.n_observed >= 1 && T.n_observed <= n &&
                  T.n_times * T.n_observed <= ABC_ODE_MAX_STATS,
              "sim_mass_action_ssa: 1 <= S = n_times * n_observed <= 256");
  ABC_REQUIRE(d >= 1 && d <= 32 && B >= 0 && ld >= B,
              "sim_mass_action_ssa: bad sizes (d <= 32)");
  ABC_REQUIRE(max_events >= 1 && max_events <= kSsaMaxEvents,
              "sim_mass_action_ssa: 1 <= max_events <= 2^24");
  ABC_REQUIRE(offset <= (uint64_t{1} << 40) &&
                  static_cast<uint64_t>(B) <= (uint64_t{1} << 40) - offset,
              "sim_mass_action_ssa: offset + B <= 2^40");
  ABC_REQUIRE(T.pair_start[0] == 0, "sim_mass_action_ssa: pair_start[0] != 0");
  for (int r = 0; r < R; ++r) {
    ABC_REQUIRE(T.rate_kind[r] >= 0 && T.rate_kind[r] <= 2,
                "sim_mass_action_ssa: rate_kind of reaction %d", r);
    ABC_REQUIRE(T.rate_kind[r] == 0 || (T.rate_col[r] >= 0 && T.rate_col[r] < d),
                "sim_mass_action_ssa: reaction %d reads theta column %d of %d", r,
                T.rate_col[r], d);
    for (int q = 0; q < 2; ++q)
      ABC_REQUIRE(T.reactant[r][q] >= -1 && T.reactant[r][q] < n,
                  "sim_mass_action_ssa: reactant of reaction %d", r);
    ABC_REQUIRE(T.pair_start[r + 1] >= T.pair_start[r] &&
                    T.pair_start[r + 1] <= ABC_ODE_MAX_PAIRS,
                "sim_mass_action_ssa: pair_start of reaction %d", r);
  }
  for (int p = 0; p < T.pair_start[R]; ++p)
    ABC_REQUIRE((T.pair[p] & 0xff) < n, "sim_mass_action_ssa: species of pair %d", p);
  for (int i = 0; i < n; ++i) {
    ABC_REQUIRE(T.x_init_col[i] >= -1 && T.x_init_col[i] < d,
                "sim_mass_action_ssa: x_init of species %d reads theta column %d of %d",
                i, T.x_init_col[i], d);
    const double v = T.x_init[i];
    ABC_REQUIRE(T.x_init_col[i] >= 0 || (v >= 0.0 && v < 2147483648.0 && v == std::rint(v)),
                "sim_mass_action_ssa: x_init of species %d must be an integer in [0, 2^31)",
                i);
  }
  for (int o = 0; o < T.n_observed; ++o)
    ABC_REQUIRE(T.observed[o] >= 0 && T.observed[o] < n,
                "sim_mass_action_ssa: observed species %d", o);
  for (int j = 0; j < T.n_times; ++j)
    ABC_REQUIRE(T.t_obs[j] > (j ? T.t_obs[j - 1] : 0.0) && std::isfinite(T.t_obs[j]),
                "sim_mass_action_ssa: t_obs must be positive and strictly increasing");
  if (B == 0) return kOk;
  ABC_REQUIRE(theta && out_T, "sim_mass_action_ssa: null pointer");

  SsaDeps D;
  for (int r = 0; r < R; ++r) {
    unsigned m = 0;
    for (int p = T.pair_start[r]; p < T.pair_start[r + 1]; ++p)
      for (int q = 0; q < R; ++q)
        if ((T.pair[p] >> 8) != 0 &&
            (T.reactant[q][0] == (T.pair[p] & 0xff) || T.reactant[q][1] == (T.pair[p] & 0xff)))
          m |= 1u << q;
    D.m[r] = static_cast<uint16_t>(m);
  }
  for (int r = R; r < ABC_ODE_MAX_REACTIONS; ++r) D.m[r] = 0;
  const SsaArgs A{theta, out_T, events_out, B, ld, max_events, seed, sid, offset, d};
  const size_t lds = static_cast<size_t>(2 * R) * kSsaBlock * sizeof(double);
  const int64_t waves = ceil_div(B, kSsaBlock);

  if (tuning_knob(kKnobSsaRefill, 0) == 0) {
    const dim3 grid(static_cast<unsigned>(waves));
#define L(N_)                                                                      \
  case N_:                                                                         \
    hipLaunchKernelGGL(ssa_plain_kernel<N_>, grid, dim3(kSsaBlock), lds, st, T, D, A); \
    break;
    switch (n) {
      L(1) L(2) L(3) L(4) L(5) L(6) L(7) L(8)
    }
#undef L
    ABC_LAUNCH_CHECK("ssa_plain_kernel");
    return kOk;
  }

  // persistent grid: ABC_SSA_GRID waves, or kSsaWavesPerCu per compute unit
  // as far as the LDS of a unit (160 KiB) holds them
  int64_t g = tuning_knob(kKnobSsaGrid, 0);
  if (g < 1) {
    static std::atomic<int> cus[64];
    int dev = 0;
    ABC_HIP(hipGetDevice(&dev));
    int c = dev < 64 ? cus[dev].load(std::memory_order_relaxed) : 0;
    if (c == 0) {
      ABC_HIP(hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev));
      if (dev < 64) cus[dev].store(c, std::memory_order_relaxed);
    }
    const int64_t fit = static_cast<int64_t>(160 * 1024 / lds);
    g = static_cast<int64_t>(c) * (fit < kSsaWavesPerCu ? fit : kSsaWavesPerCu);
  }
  const dim3 grid(static_cast<unsigned>(g < waves ? g : waves));
  // the claim counter of this call: slots are handed out in turn, so a call
  // meets another one's counter only with kSsaSlots calls in flight on one
  // device.  Cleared by a kernel, not a memset node: the pair is capturable.
  static std::atomic<unsigned> next_slot{0};
  const int slot = static_cast<int>(next_slot.fetch_add(1, std::memory_order_relaxed) % kSsaSlots);
  hipLaunchKernelGGL(ssa_zero_kernel, dim3(1), dim3(1), 0, st, slot);
#define L(N_)                                                                     \
  case N_:                                                                        \
    hipLaunchKernelGGL(ssa_refill_kernel<N_>, grid, dim3(kSsaBlock), lds, st, T, D, A, \
                       slot);                                                     \
    break;
  switch (n) {
    L(1) L(2) L(3) L(4) L(5) L(6) L(7) L(8)
  }
#undef L
  ABC_LAUNCH_CHECK("ssa_refill_kernel");
  return kOk;
}

}  // extern "C"

namespace abc {
int preload_sim_ssa() { return preload_kernel(ssa_plain_kernel<2>); }
}  // namespace abc
