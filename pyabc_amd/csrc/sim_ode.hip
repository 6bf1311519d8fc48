// Mass-action reaction-network ODE batch model (MassActionODEModel): the
// model class of the reference's worked examples (conversion_reaction.ipynb,
// noise.ipynb), where the model is scipy's odeint inside a Python function.
//
//   dx/dt = sum_r nu_r * k_r * prod_{reactant slots of r} x
//
// One lane integrates one proposal with the Dormand-Prince 5(4) pair under
// scipy RK45's step controller; the wave leaves an observation interval when
// its last lane has reached the observation time (the divergent step loop is
// an EXEC-mask loop: a wave vote per iteration, finished lanes idle), so the
// statistics of one time are stored by the whole wave at once, coalesced.
//
// Where the data lives ("Mass-action ODE model"):
//   * the network table is a kernel argument BY VALUE (3160 bytes of the
//     4 KiB argument segment): every read of it is a scalar load with a
//     wave-uniform index, its values sit in SGPRs, and the species selects
//     below are scalar compares -- a copy staged in LDS would come back in
//     VGPRs that the compiler cannot know to be uniform;
//   * state, the seven stage derivatives, the trial state and the error live
//     in VGPRs: every loop over species is unrolled over the template
//     parameter N and a wave-uniform species index i is resolved by a select
//     chain (pick / the scatter in rhs), never by indexing a private array;
//   * the per-lane rates k_r (10 ** theta where asked) are evaluated once
//     and parked in LDS, [r][lane], 8 R bytes per lane: they are the one
//     per-lane array whose index r is a run-time value, and 16 of them in
//     registers would cost the n = 8 instantiation 32 VGPRs.  Each lane reads
//     back only what it wrote: no barrier.
// No matrix instructions: n <= 8 with a sparse stoichiometry and a step size
// per lane leaves no dense tile to feed them.
#include "common.hpp"
#include "philox.hpp"
#include "../../include/abc_hip.h"

namespace abc {

static_assert(sizeof(abc_ode_table) == 3160, "abc_ode_table layout (abc_hip.h)");

constexpr int kOdeBlock = 64;  // one wave: a block retires with its slowest lane

// x[i] for a wave-uniform i in [0, N)
template <int N>
__device__ __forceinline__ double pick(const double (&x)[N], int i) {
  double r = 0.0;
#pragma unroll
  for (int k = 0; k < N; ++k) r = i == k ? x[k] : r;
  return r;
}

// dx = f(x): per reaction one LDS read (its rate), up to two selects and
// products, and one fma per non-zero net coefficient
template <int N>
__device__ __forceinline__ void rhs(const abc_ode_table& T, const double* kl,
                                    const double (&x)[N], double (&dx)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) dx[i] = 0.0;
  const int R = T.n_reactions;
  for (int r = 0; r < R; ++r) {
    double v = kl[r * kOdeBlock];
    const int a = T.reactant[r][0], c = T.reactant[r][1];
    if (a >= 0) v *= pick<N>(x, a);
    if (c >= 0) v *= pick<N>(x, c);
    const int p1 = T.pair_start[r + 1];
    for (int p = T.pair_start[r]; p < p1; ++p) {
      const int e = T.pair[p];
      const int sp = e & 0xff;
      const double nu = static_cast<double>(e >> 8);
#pragma unroll
      for (int i = 0; i < N; ++i)
        if (sp == i) dx[i] = fma(nu, v, dx[i]);
    }
  }
}

// RMS over species of v / (atol + rtol * m)
template <int N>
__device__ __forceinline__ double rms_scaled(const double (&v)[N],
                                             const double (&m)[N], double rtol,
                                             double atol) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double q = v[i] / fma(rtol, m[i], atol);
    s = fma(q, q, s);
  }
  return sqrt(s * (1.0 / N));
}

// 0.9 * e ** -0.2 on the fp32 transcendental unit (v_log_f32, v_exp_f32):
// the controller's factor is a heuristic that no result resolves beyond a
// few digits; e = 0 or a denormal float gives +inf, e = inf gives 0, and the
// caller clamps
__device__ __forceinline__ double step_factor(double e) {
  const float l = __builtin_amdgcn_logf(static_cast<float>(e));
  return 0.9 * static_cast<double>(__builtin_amdgcn_exp2f(-0.2f * l));
}

__device__ __forceinline__ bool is_finite(double v) { return fabs(v) < INFINITY; }

template <int N>
__global__ __launch_bounds__(kOdeBlock) void mass_action_ode_kernel(
    const abc_ode_table T, const double* __restrict__ theta, int64_t B, int d,
    double rtol, double atol, int64_t max_steps, double sigma, uint64_t seed,
    uint64_t sid, uint64_t offset, double* __restrict__ out_T, int64_t ld,
    int64_t* __restrict__ steps_out) {
  extern __shared__ double k_lds[];  // [R][kOdeBlock]
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kOdeBlock + threadIdx.x;
  if (b >= B) return;  // no barrier below
  const double* kl = k_lds + threadIdx.x;
  const double* th = theta + b * d;
  const int R = T.n_reactions;
  for (int r = 0; r < R; ++r) {
    const int kind = T.rate_kind[r];
    double k = T.rate_const[r];
    if (kind != 0) {
      k = th[T.rate_col[r]];
      if (kind == 2) k = exp10(k);
    }
    k_lds[r * kOdeBlock + threadIdx.x] = k;
  }
  double x[N], k1[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int col = T.x_init_col[i];
    x[i] = col < 0 ? T.x_init[i] : th[col];
  }
  rhs<N>(T, kl, x, k1);

  // first step (Hairer, Norsett, Wanner I, II.4; scipy select_initial_step)
  double h_abs;
  {
    double ax[N], y1[N], f1[N];
#pragma unroll
    for (int i = 0; i < N; ++i) ax[i] = fabs(x[i]);
    const double d0 = rms_scaled<N>(x, ax, rtol, atol);
    const double d1 = rms_scaled<N>(k1, ax, rtol, atol);
    const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
#pragma unroll
    for (int i = 0; i < N; ++i) y1[i] = fma(h0, k1[i], x[i]);
    rhs<N>(T, kl, y1, f1);
#pragma unroll
    for (int i = 0; i < N; ++i) f1[i] -= k1[i];
    const double d2 = rms_scaled<N>(f1, ax, rtol, atol) / h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15)
                          ? fmax(1e-6, h0 * 1e-3)
                          : pow(0.01 / fmax(d1, d2), 0.2);
    h_abs = fmin(100.0 * h0, h1);
  }

  double t = 0.0;
  int64_t steps = 0;
  bool failed = false, rejected = false;
  const int n_times = T.n_times, n_obs = T.n_observed;
  const int S = n_times * n_obs;
  const uint64_t zbase = (offset + static_cast<uint64_t>(b)) * static_cast<uint64_t>(S);

  for (int j = 0; j < n_times; ++j) {
    const double tj = T.t_obs[j];
    while (!failed && t < tj) {
      // 10 ulp of t (scipy's min_step); also catches a NaN step
      const double min_step = 10.0 * (nextafter(t, INFINITY) - t);
      if (++steps > max_steps || !(h_abs >= min_step)) {
        failed = true;
        break;
      }
      const double left = tj - t;
      const bool clipped = h_abs >= left;
      const double h = clipped ? left : h_abs;
      double y[N], k2[N], k3[N], k4[N], k5[N], k6[N], k7[N];
#pragma unroll
      for (int i = 0; i < N; ++i) y[i] = fma(h * (1.0 / 5.0), k1[i], x[i]);
      rhs<N>(T, kl, y, k2);
#pragma unroll
      for (int i = 0; i < N; ++i)
        y[i] = fma(h, fma(9.0 / 40.0, k2[i], 3.0 / 40.0 * k1[i]), x[i]);
      rhs<N>(T, kl, y, k3);
#pragma unroll
      for (int i = 0; i < N; ++i)
        y[i] = fma(h,
                   fma(32.0 / 9.0, k3[i],
                       fma(-56.0 / 15.0, k2[i], 44.0 / 45.0 * k1[i])),
                   x[i]);
      rhs<N>(T, kl, y, k4);
#pragma unroll
      for (int i = 0; i < N; ++i)
        y[i] = fma(h,
                   fma(-212.0 / 729.0, k4[i],
                       fma(64448.0 / 6561.0, k3[i],
                           fma(-25360.0 / 2187.0, k2[i],
                               19372.0 / 6561.0 * k1[i]))),
                   x[i]);
      rhs<N>(T, kl, y, k5);
#pragma unroll
      for (int i = 0; i < N; ++i)
        y[i] = fma(h,
                   fma(-5103.0 / 18656.0, k5[i],
                       fma(49.0 / 176.0, k4[i],
                           fma(46732.0 / 5247.0, k3[i],
                               fma(-355.0 / 33.0, k2[i],
                                   9017.0 / 3168.0 * k1[i])))),
                   x[i]);
      rhs<N>(T, kl, y, k6);
      // the fifth-order solution, whose derivative is the next first stage
#pragma unroll
      for (int i = 0; i < N; ++i)
        y[i] = fma(h,
                   fma(11.0 / 84.0, k6[i],
                       fma(-2187.0 / 6784.0, k5[i],
                           fma(125.0 / 192.0, k4[i],
                               fma(500.0 / 1113.0, k3[i],
                                   35.0 / 384.0 * k1[i])))),
                   x[i]);
      rhs<N>(T, kl, y, k7);
      double err[N], mx[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        err[i] = h * fma(1.0 / 40.0, k7[i],
                         fma(-22.0 / 525.0, k6[i],
                             fma(17253.0 / 339200.0, k5[i],
                                 fma(-71.0 / 1920.0, k4[i],
                                     fma(71.0 / 16695.0, k3[i],
                                         -71.0 / 57600.0 * k1[i])))));
        mx[i] = fmax(fabs(x[i]), fabs(y[i]));
      }
      const double en = rms_scaled<N>(err, mx, rtol, atol);
      if (!is_finite(en)) {
        failed = true;
        break;
      }
      if (en < 1.0) {
        double f = fmin(10.0, step_factor(en));
        if (rejected) f = fmin(1.0, f);
        // a step cut short by the observation time says nothing against the
        // step size it was cut from
        h_abs = clipped ? fmax(h * f, h_abs) : h * f;
        t = clipped ? tj : t + h;
        rejected = false;
#pragma unroll
        for (int i = 0; i < N; ++i) {
          x[i] = y[i];
          k1[i] = k7[i];
        }
      } else {
        h_abs = h * fmax(0.2, step_factor(en));
        rejected = true;
      }
    }
    // the wave is together again: row o * n_times + j, lanes along b
    for (int o = 0; o < n_obs; ++o) {
      double v = pick<N>(x, T.observed[o]);
      const int s = o * n_times + j;
      if (sigma != 0.0) {
        const uint64_t zi = zbase + static_cast<uint64_t>(s);
        float z4[4];
        box_muller4_f32(philox_block(seed, sid, zi >> 2), z4);
        const int m = static_cast<int>(zi & 3);
        const float z = m == 0 ? z4[0] : m == 1 ? z4[1] : m == 2 ? z4[2] : z4[3];
        v = fma(sigma, static_cast<double>(z), v);
      }
      out_T[static_cast<int64_t>(s) * ld + b] = failed ? INFINITY : v;
    }
  }
  // a lane that failed in interval j wrote finite values for the times
  // before it: the whole column becomes +inf
  if (failed)
    for (int s = 0; s < S; ++s) out_T[static_cast<int64_t>(s) * ld + b] = INFINITY;
  if (steps_out) steps_out[b] = steps;
}

}  // namespace abc

using namespace abc;

extern "C" {

int abc_sim_mass_action_ode_f64(const abc_ode_table* table, const double* theta,
                                int64_t B, int d, double rtol, double atol,
                                int64_t max_steps, double sigma, uint64_t seed,
                                uint64_t sid, uint64_t offset, double* out_T,
                                int64_t ld, int64_t* steps_out, hipStream_t st) {
  ABC_REQUIRE(table, "sim_mass_action_ode: null table");
  const abc_ode_table& T = *table;
  const int n = T.n_species, R = T.n_reactions;
  ABC_REQUIRE(n >= 1 && n <= ABC_ODE_MAX_SPECIES,
              "sim_mass_action_ode: 1 <= n_species <= 8");
  ABC_REQUIRE(R >= 1 && R <= ABC_ODE_MAX_REACTIONS,
              "sim_mass_action_ode: 1 <= n_reactions <= 16");
  ABC_REQUIRE(T.n_times >= 1 && T.n_observed >= 1 && T.n_observed <= n &&
                  T.n_times * T.n_observed <= ABC_ODE_MAX_STATS,
              "sim_mass_action_ode: 1 <= S = n_times * n_observed <= 256");
  ABC_REQUIRE(d >= 1 && d <= 32 && B >= 0 && ld >= B,
              "sim_mass_action_ode: bad sizes (d <= 32)");
  ABC_REQUIRE(rtol > 0.0 && atol >= 0.0 && max_steps >= 1 && std::isfinite(sigma),
              "sim_mass_action_ode: rtol > 0, atol >= 0, max_steps >= 1");
  ABC_REQUIRE(T.pair_start[0] == 0, "sim_mass_action_ode: pair_start[0] != 0");
  for (int r = 0; r < R; ++r) {
    ABC_REQUIRE(T.rate_kind[r] >= 0 && T.rate_kind[r] <= 2,
                "sim_mass_action_ode: rate_kind of reaction %d", r);
    ABC_REQUIRE(T.rate_kind[r] == 0 || (T.rate_col[r] >= 0 && T.rate_col[r] < d),
                "sim_mass_action_ode: reaction %d reads theta column %d of %d", r,
                T.rate_col[r], d);
    for (int q = 0; q < 2; ++q)
      ABC_REQUIRE(T.reactant[r][q] >= -1 && T.reactant[r][q] < n,
                  "sim_mass_action_ode: reactant of reaction %d", r);
    ABC_REQUIRE(T.pair_start[r + 1] >= T.pair_start[r] &&
                    T.pair_start[r + 1] <= ABC_ODE_MAX_PAIRS,
                "sim_mass_action_ode: pair_start of reaction %d", r);
  }
  for (int p = 0; p < T.pair_start[R]; ++p)
    ABC_REQUIRE((T.pair[p] & 0xff) < n, "sim_mass_action_ode: species of pair %d", p);
  for (int i = 0; i < n; ++i)
    ABC_REQUIRE(T.x_init_col[i] >= -1 && T.x_init_col[i] < d,
                "sim_mass_action_ode: x_init of species %d reads theta column %d of %d",
                i, T.x_init_col[i], d);
  for (int o = 0; o < T.n_observed; ++o)
    ABC_REQUIRE(T.observed[o] >= 0 && T.observed[o] < n,
                "sim_mass_action_ode: observed species %d", o);
  for (int j = 0; j < T.n_times; ++j)
    ABC_REQUIRE(T.t_obs[j] > (j ? T.t_obs[j - 1] : 0.0) && std::isfinite(T.t_obs[j]),
                "sim_mass_action_ode: t_obs must be positive and strictly increasing");
  if (B == 0) return kOk;
  ABC_REQUIRE(theta && out_T, "sim_mass_action_ode: null pointer");
  const dim3 grid(static_cast<unsigned>(ceil_div(B, kOdeBlock)));
  const size_t lds = static_cast<size_t>(R) * kOdeBlock * sizeof(double);
#define L(N_)                                                                   \
  case N_:                                                                      \
    hipLaunchKernelGGL(mass_action_ode_kernel<N_>, grid, dim3(kOdeBlock), lds,  \
                       st, T, theta, B, d, rtol, atol, max_steps, sigma, seed,  \
                       sid, offset, out_T, ld, steps_out);                      \
    break;
  switch (n) {
    L(1) L(2) L(3) L(4) L(5) L(6) L(7) L(8)
  }
#undef L
  ABC_LAUNCH_CHECK("mass_action_ode_kernel");
  return kOk;
}

}  // extern "C"

namespace abc {
int preload_sim_ode() { return preload_kernel(mass_action_ode_kernel<2>); }
}  // namespace abc
