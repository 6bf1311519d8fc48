"""Per-kernel roofline table on the GPU (one MI355X).

Times every hot-path entry point of libabc_hip at the BASELINE.json config
sizes with HIP events on the stream the kernels are launched on (torch's
current stream), and prices each against its roofline with the algorithmic
bytes / flops per unit of SURVEY.md 8(d) (DESIGN.md restates them):

  HBM-bound kernels:  frac = (units * bytes_per_unit / t) / 8.0 TB/s
  VALU-bound kernels: frac = (units * flops_per_unit / t) / 157.3 TF (f32)
                      or / 78.6 TF (f64)

    python tools/bench_kernels.py [--quick] > gpurun_out/kernels.jsonl
"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyabc_amd import kernels as K  # noqa: E402
from pyabc_amd._native import call as nat_call  # noqa: E402
from pyabc_amd.engine import DeviceMVNFit  # noqa: E402

HBM = 8.0e12
FP32 = 157.3e12
FP64 = 78.6e12
F64 = torch.float64


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    best = math.inf
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / 1e3)
    return best


def report(name, t, units, unit, per_unit, bound, extra=None):
    if bound == "hbm":
        ach = units * per_unit / t
        peak = HBM
        u = "GB/s"
        scale = 1e9
    else:
        ach = units * per_unit / t
        peak = FP32 if bound == "valu_f32" else FP64
        u = "TFLOP/s"
        scale = 1e12
    row = {"kernel": name, "ms": t * 1e3, "units": units, "unit": unit,
           "per_unit": per_unit, "bound": bound,
           "achieved": ach / scale, "peak": peak / scale, "ach_unit": u,
           "frac": ach / peak, "units_per_s": units / t}
    if extra:
        row.update(extra)
    print(json.dumps(row), flush=True)
    return row


def bench_normal_kernel(B=1 << 20, calls=20):
    """abc_normal_kernel_f64 with the fused acceptance, alone: `calls`
    launches between two events (the allocations of the outputs overlap the
    previous launch), best of 5.  2 S R FLOP against the measured MFMA rate
    (tools/probes/mfma_f64_rate.hip) and 8 S + 18 bytes against HBM."""
    g = torch.Generator(device="cuda").manual_seed(3)
    for S in (64, 256):
        R = S
        stats = torch.randn((S, B), dtype=F64, device="cuda", generator=g)
        x0 = torch.randn(S, dtype=F64, device="cuda", generator=g)
        U = torch.randn((S, R), dtype=F64, device="cuda", generator=g) / S ** 0.5

        def run():
            for _ in range(calls):
                K.normal_kernel(stats, x0, U, 1.0, pdf_norm=-0.5 * S,
                                inv_temp=0.1, seed=1, stream=9)
        t = timed(run) / calls
        report("normal_kernel_accept_f64", t, B, "evaluations", 2 * S * R,
               "mfma_f64", {"S": S, "R": R, "mfma_probe_tflops": 43.0,
                            "bytes_per_eval": 8 * S + 18,
                            "GB_per_s": B * (8 * S + 18) / t / 1e9})
        del stats


def bench_kde_cv(n=100_000, d=8, k=5, G=5):
    """abc_kde_cv_f64 alone (whitening, pair pass and merge of one call)
    against the same search with the single-bandwidth entry points: k G times
    DeviceMVNFit on the gathered training rows plus logpdf on the fold."""
    from pyabc_amd.transition import kfold_offsets
    g = torch.Generator(device="cuda").manual_seed(5)
    X = torch.randn((n, d), dtype=F64, device="cuda", generator=g)
    w = torch.rand(n, dtype=F64, device="cuda", generator=g) + 0.5
    w /= w.sum()
    off = kfold_offsets(n, k)
    grid = np.linspace(0.05, 1.0, G)
    mu = X.mean(0).repeat(k, 1)
    Us = (torch.eye(d, dtype=F64, device="cuda") * 4.0).repeat(k, 1, 1)
    pairs = sum((n - (off[f + 1] - off[f])) * (off[f + 1] - off[f])
                for f in range(k))
    t = timed(lambda: K.kde_cv(X, w, off, mu, Us, grid), reps=3)
    # per pair: 2 d (Gram) + 3, per pair and grid value ~8 (exponent twice,
    # maximum, shift, exponential, sum)
    report("kde_cv_f64", t, pairs * G, "pair_grid_values", 8 + (2 * d + 3) / G,
           "valu_f64", {"n": n, "d": d, "k": k, "G": G, "pairs": pairs})

    def loop():
        out = torch.empty((k, G), dtype=F64, device="cuda")
        for f in range(k):
            lo, hi = off[f], off[f + 1]
            Xtr, wtr = torch.cat([X[:lo], X[hi:]]), torch.cat([w[:lo], w[hi:]])
            for j, s in enumerate(grid):
                fit = DeviceMVNFit(Xtr, wtr, s)
                out[f, j] = (fit.logpdf(X[lo:hi]) * w[lo:hi]).sum()
        return out
    t2 = timed(loop, reps=3)
    report("kde_cv_by_single_fits", t2, pairs * G, "pair_grid_values", 0.0,
           "valu_f64", {"n": n, "d": d, "k": k, "G": G,
                        "ratio_to_kde_cv": t2 / t})


def bench_count_kernel(B=1 << 20, calls=10):
    """abc_count_kernel_f64 with the fused acceptance, alone, per kind at
    S = 16 and 256, once with every count below the table size T = 4096 (LDS
    table branch) and once with every count above it (Stirling / log branch).
    Reports the element rate (S B / t), the HBM rate its 8 S + 18 bytes per
    evaluation imply, and for the table branch the fp64 instruction rate from
    the per-element count read off the source (trunc, subtractions, two
    TwoSums and their compensation adds: 17 binomial, 18 negative binomial;
    trunc, fma, add: 3 Poisson).  The Stirling branch's libm log is not
    counted, so that row carries no instruction rate."""
    g = torch.Generator(device="cuda").manual_seed(4)
    ops = {K.KERNEL_BINOMIAL: 17, K.KERNEL_POISSON: 3, K.KERNEL_NEGBINOMIAL: 18}
    K.count_table()
    for S in (16, 256):
        x0 = torch.randint(1, 40, (S,), device="cuda", generator=g).to(F64)
        for branch, lo, hi in (("table", 40, 2000), ("stirling", 5000, 10 ** 6)):
            stats = torch.randint(lo, hi, (S, B), device="cuda",
                                  generator=g).to(F64)
            for kind, name in ((K.KERNEL_BINOMIAL, "binomial"),
                               (K.KERNEL_POISSON, "poisson"),
                               (K.KERNEL_NEGBINOMIAL, "negbinomial")):
                def run():
                    for _ in range(calls):
                        K.count_kernel(stats, x0, 0.3, kind, pdf_norm=-3.0 * S,
                                       inv_temp=0.1, seed=1, stream=9)
                t = timed(run) / calls
                extra = {"S": S, "kind": name, "branch": branch,
                         "elements_per_s": S * B / t}
                if branch == "table":
                    extra["fp64_Tops_per_s"] = S * B * ops[kind] / t / 1e12
                report("count_kernel_accept_f64", t, B, "evaluations",
                       8 * S + 18, "hbm", extra)
            del stats


def bench_sim_ode(B=1 << 20, calls=40, host_rows=512):
    """abc_sim_mass_action_ode_f64 on the conversion reaction A <-> B
    (log10 k uniform in [-1, 0.5], ten observation times up to t = 30, the
    model's default tolerances): `calls` launches between two events, best
    of 5; the right-hand-side evaluations are 2 + 6 attempted steps per
    proposal, from the kernel's own step counts.  The CPU figure beside it is
    simulate_host (scipy RK45, one thread) on the first `host_rows` rows."""
    import time
    from pyabc_amd.batch_models import MassActionODEModel
    model = MassActionODEModel(
        ["A", "B"], [({"A": 1}, {"B": 1}, ("log10theta", 0)),
                     ({"B": 1}, {"A": 1}, ("log10theta", 1))],
        [1.0, 0.0], np.linspace(3, 30, 10))
    g = torch.Generator(device="cuda").manual_seed(6)
    theta = torch.rand((B, 2), dtype=F64, device="cuda", generator=g) * 1.5 - 1
    steps = torch.empty(B, dtype=torch.int64, device="cuda")
    out = K.sim_mass_action_ode(theta, model.table, model.rtol, model.atol,
                                model.max_steps, 0.0, 1, 3, 0, steps_out=steps)
    rhs = 2 * B + 6 * int(steps.sum())

    def run():
        for _ in range(calls):
            K.sim_mass_action_ode(theta, model.table, model.rtol, model.atol,
                                  model.max_steps, 0.0, 1, 3, 0, out_T=out)
    t = timed(run) / calls
    th = theta[:host_rows].cpu().numpy()
    t0 = time.perf_counter()
    model.simulate_host(th)
    t_host = (time.perf_counter() - t0) / host_rows
    print(json.dumps({
        "kernel": "sim_mass_action_ode_f64", "network": "conv", "ms": t * 1e3,
        "units": B, "unit": "proposals", "units_per_s": B / t,
        "rhs_evals_per_s": rhs / t, "mean_steps": float(steps.sum()) / B,
        "max_steps": int(steps.max()), "failed": int(torch.isinf(out[0]).sum()),
        "host_proposals_per_s": 1 / t_host, "host_rows": host_rows}),
        flush=True)


def bench_prior(B=1 << 22, d=8, calls=20, reps=3):
    """abc_prior_logpdf_f64 / abc_prior_rvs_f64 at B rows of d marginals for
    an all-normal and an all-beta table (`calls` launches between two
    events, best of 5), then config 1 of tools/bench_configs.py with a
    normal prior beside the same config with its uniform prior, alternated
    `reps` times in this process: the median generation (t >= 1) of each, and
    the prior passes of one normal-prior generation (the support flags of a
    round's proposals, the densities of the accepted rows) timed alone at
    that config's shapes as a share of that generation."""
    import contextlib
    import io
    import pyabc_amd as pa
    from tools import bench_configs as bc
    for name, rv in (("norm", pa.RV("norm", 1.0, 2.0)),
                     ("beta", pa.RV("beta", 2.0, 5.0))):
        table = pa.Distribution(
            **{f"p{i}": rv for i in range(d)}).device_table()[1]
        theta = K.prior_rvs(table, d, 1, 2, 0, B)
        lp = torch.empty(B, dtype=F64, device="cuda")
        pd = torch.empty(B, dtype=F64, device="cuda")
        sup = torch.empty(B, dtype=torch.uint8, device="cuda")

        def run_pdf():
            for _ in range(calls):
                nat_call("abc_prior_logpdf_f64", K.ptr(theta),
                         ctypes.byref(table), d, B, K.ptr(lp), K.ptr(pd),
                         K.ptr(sup), K.nat.stream())

        def run_rvs():
            for _ in range(calls):
                nat_call("abc_prior_rvs_f64", ctypes.byref(table), d, 1, 2, 0,
                         B, K.ptr(theta), K.nat.stream())
        for kern, fn, nbytes in (("prior_logpdf_f64", run_pdf, 8 * d + 17),
                                 ("prior_rvs_f64", run_rvs, 8 * d)):
            t = timed(fn) / calls
            print(json.dumps({"kernel": kern, "table": name, "B": B, "d": d,
                              "ms": t * 1e3, "rows_per_s": B / t,
                              "hbm_GB_per_s": B * nbytes / t / 1e9}),
                  flush=True)

    def c1(prior):
        np.random.seed(0)
        abc = pa.ABCSMC(pa.GaussianMeanModel(), prior, pa.PNormDistance(p=2),
                        population_size=1000, eps=pa.MedianEpsilon(),
                        sampler=pa.GPUBatchSampler(seed=1))
        with contextlib.redirect_stdout(io.StringIO()):
            out = bc.run("c1", abc, {"data": 2.5}, ["mean"], [2.5],
                         minimum_epsilon=0.1, max_nr_populations=10)
        assert out["all_batch"]
        return out["generation_ms_median_t_ge_1"], abc.sampler.min_batch
    priors = {"uniform": pa.Distribution(mean=pa.RV("uniform", 0, 5)),
              "norm": pa.Distribution(mean=pa.RV("norm", 2.5, 1.5))}
    ms = {k: [] for k in priors}
    for _ in range(reps + 1):          # the first pass warms both up
        for k, prior in priors.items():
            g, min_batch = c1(prior)
            ms[k].append(g)
    table = priors["norm"].device_table()[1]
    prop = K.prior_rvs(table, 1, 1, 2, 0, min_batch)
    t_sup = timed(lambda: K.prior_logpdf(prop, table, logp=False, pd=False))
    t_pd = timed(lambda: K.prior_logpdf(prop[:1000], table, logp=False,
                                        support=False))
    med = {k: float(np.median(v[1:])) for k, v in ms.items()}
    print(json.dumps({
        "config": "c1_quickstart_N1000", "generation_ms_uniform": med["uniform"],
        "generation_ms_norm": med["norm"], "runs_ms": ms,
        "prior_support_pass_ms": t_sup * 1e3, "prior_density_pass_ms": t_pd * 1e3,
        "prior_share_of_generation": (t_sup + t_pd) * 1e3 / med["norm"]}),
        flush=True)


def bench_sim_ssa(B=1 << 20, calls=10, reps=7, host_rows=256):
    """abc_sim_mass_action_ssa_f64 on pyABC's chemical-reaction model 1 (X + Y
    -> 2Y from (40, 3), twenty observation times up to 0.1): a skewed batch
    (log10 k uniform over [-0.5, 1.5]) and a homogeneous one (k = 2.3 in every
    row), each in the plain form, the refill form at its default grid and at
    8 and 32 waves per compute unit.  The forms alternate within one process;
    a row reports the median of `reps` windows of `calls` launches and their
    spread (max - min) / median, the figure a difference between two forms
    has to exceed.  Events are the kernel's own counts.  The CPU figure is
    simulate_host on the first `host_rows` rows of the skewed batch."""
    import os
    import time
    from pyabc_amd.batch_models import MassActionSSAModel
    model = MassActionSSAModel(
        ["X", "Y"], [({"X": 1, "Y": 1}, {"Y": 2}, ("log10theta", 0))],
        [40, 3], np.linspace(0.005, 0.1, 20))
    g = torch.Generator(device="cuda").manual_seed(6)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    forms = {"plain": (0, None), "refill": (1, None),
             "refill_8_per_cu": (1, 8 * cus), "refill_32_per_cu": (1, 32 * cus)}

    def select(refill, grid):
        os.environ["ABC_SSA_REFILL"] = str(refill)
        os.environ.pop("ABC_SSA_GRID", None)
        if grid:
            os.environ["ABC_SSA_GRID"] = str(grid)
        K.reload_tuning()

    batches = {
        "skewed": torch.rand((B, 1), dtype=F64, device="cuda", generator=g) * 2 - 0.5,
        "homogeneous": torch.full((B, 1), float(np.log10(2.3)), dtype=F64,
                                  device="cuda")}
    for bname, theta in batches.items():
        ev = torch.empty(B, dtype=torch.int64, device="cuda")
        select(0, None)
        want = K.sim_mass_action_ssa(theta, model.table, model.max_events, 1, 3,
                                     0, events_out=ev)
        events = int(ev.sum())
        out = torch.empty_like(want)
        ms = {f: [] for f in forms}
        for rep in range(reps + 1):         # the first round warms up
            for f, (refill, grid) in forms.items():
                select(refill, grid)
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    K.sim_mass_action_ssa(theta, model.table, model.max_events,
                                          1, 3, 0, out_T=out)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    ms[f].append(e0.elapsed_time(e1) / calls)
                else:
                    assert torch.equal(out, want), f
        for f, v in ms.items():
            t = float(np.median(v)) * 1e-3
            print(json.dumps({
                "kernel": "sim_mass_action_ssa_f64", "network": "chem",
                "batch": bname, "form": f, "ms": t * 1e3,
                "spread": (max(v) - min(v)) / float(np.median(v)),
                "units": B, "unit": "proposals", "units_per_s": B / t,
                "events_per_s": events / t, "mean_events": events / B,
                "max_events": int(ev.max())}), flush=True)
    os.environ.pop("ABC_SSA_REFILL", None)
    os.environ.pop("ABC_SSA_GRID", None)
    K.reload_tuning()
    th = batches["skewed"][:host_rows].cpu().numpy()
    u = np.random.default_rng(0).uniform(size=(host_rows, 128))
    t0 = time.perf_counter()
    _, hev, _ = model.simulate_host(th, u, info=True)
    t_host = time.perf_counter() - t0
    print(json.dumps({"kernel": "simulate_host", "network": "chem",
                      "host_proposals_per_s": host_rows / t_host,
                      "host_events_per_s": int(hev.sum()) / t_host,
                      "host_rows": host_rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--normal-kernel", action="store_true",
                    help="only the full-covariance normal kernel's rows")
    ap.add_argument("--kde-cv", action="store_true",
                    help="only the cross-validation kernel and its "
                         "single-fit equivalent")
    ap.add_argument("--count-kernel", action="store_true",
                    help="only the count-data kernels' rows")
    ap.add_argument("--sim-ode", action="store_true",
                    help="only the mass-action ODE model's row")
    ap.add_argument("--sim-ssa", action="store_true",
                    help="only the mass-action SSA model's rows: both launch "
                         "forms on a skewed and a homogeneous batch")
    ap.add_argument("--prior", action="store_true",
                    help="only the prior table's kernels and config 1 with a "
                         "normal prior")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.prior:
        bench_prior()
        return
    if args.sim_ode:
        bench_sim_ode()
        return
    if args.sim_ssa:
        bench_sim_ssa()
        return
    if args.normal_kernel:
        bench_normal_kernel()
        return
    if args.kde_cv:
        bench_kde_cv()
        return
    if args.count_kernel:
        bench_count_kernel()
        return
    g = torch.Generator(device="cuda").manual_seed(0)
    q = 4 if args.quick else 1

    # ---------------- (a3) KDE weight pass -------------------------------
    for (N, d, prec) in [(1_000_000 // q, 8, "mfma"), (1_000_000 // q, 8, "f32"),
                         (1_000_000 // q, 20, "mfma"), (100_000, 4, "mfma"),
                         (200_000 // q, 8, "f64")]:
        X = torch.randn((N, d), dtype=F64, device="cuda", generator=g)
        w = torch.rand(N, dtype=F64, device="cuda", generator=g) + 0.5
        w /= w.sum()
        fit = DeviceMVNFit(X, w, precision=prec)
        theta = X + 0.05 * torch.randn((N, d), dtype=F64, device="cuda",
                                       generator=g)
        Y = fit.packed.whiten(theta)
        t = timed(lambda: fit.packed.logpdf_whitened(Y), reps=3)
        pairs = N * fit.packed.npad
        if prec == "mfma":
            # priced against its own SIMD issue ceiling (bench.py
            # kde_roofline: PMC per-tile counts at d = 8, static otherwise)
            import bench
            tiles = (K.nat.lib().abc_kde_mfma_new_rows(N, d) // 32) * \
                (fit.packed.npad // 32)
            ach = (3 * d + 4) * pairs / t / 1e12
            rl = bench.kde_roofline(d, ach, None, None, t, pairs, tiles)
            print(json.dumps({
                "kernel": "kde_logpdf_mfma", "ms": t * 1e3, "units": pairs,
                "unit": "pairs", "per_unit": 3 * d + 4, "bound": "valu_issue",
                "achieved": ach, "peak": rl["peak"], "ach_unit": "TFLOP/s",
                "frac": rl["frac"], "units_per_s": pairs / t,
                "ceiling_ms": rl["ceiling_ms"],
                "probe_ns_per_tile_per_simd": rl["probe_ns_per_tile_per_simd"],
                "static_cycles_per_tile": rl["static_issue"]["cycles_per_tile"],
                "valu_equiv_frac_fp32": rl["valu_equiv"]["frac"],
                "mfma_f16_frac": rl["mfma_f16"]["frac"],
                "N": N, "M": N, "d": d}), flush=True)
            continue
        report(f"kde_logpdf_{prec}", t, pairs, "pairs", 3 * d + 4,
               "valu_f64" if prec == "f64" else "valu_f32",
               {"N": N, "M": N, "d": d})

    # ---------------- (a1) fit: weighted moments -------------------------
    N, d = 1_000_000, 8
    X = torch.randn((N, d), dtype=F64, device="cuda", generator=g)
    w = torch.rand(N, dtype=F64, device="cuda", generator=g)
    t = timed(lambda: K.weighted_moments(X, w))
    report("weighted_moments_f64", t, N, "particles", 8 * (d + 1), "hbm",
           {"d": d})

    # ---------------- (a2) resample + perturb -----------------------------
    cdf = K.resample_cdf(w)
    t = timed(lambda: K.resample_cdf(w))
    report("resample_cdf_f64", t, N, "weights", 16, "hbm")
    fit = DeviceMVNFit(X, w / w.sum())
    lo = torch.full((d,), -5.0, dtype=F64, device="cuda")
    sc = torch.full((d,), 10.0, dtype=F64, device="cuda")
    B = 1 << 21
    out = (torch.empty((B, d), dtype=F64, device="cuda"),
           torch.empty(B, dtype=torch.int64, device="cuda"),
           torch.empty(B, dtype=torch.uint8, device="cuda"))
    t = timed(lambda: K.propose_philox(fit.X, cdf, fit.A, lo, sc, 1, 2, 0, B,
                                       out=out))
    # in-kernel Philox: cdf hit 8 + X[idx] 8d + theta 8d + idx 8 + flag 1
    report("propose_philox_f64", t, B, "proposals", 16 * d + 17, "hbm",
           {"N": N, "d": d})
    tab = K.cdf_index(cdf)
    t = timed(lambda: K.propose_philox(fit.X, cdf, fit.A, lo, sc, 1, 2, 0, B,
                                       out=out, tab=tab))
    report("propose_philox_indexed_f64", t, B, "proposals", 16 * d + 17,
           "hbm", {"N": N, "d": d, "log2k": K.CDF_INDEX_LOG2})
    vpos, _ = K.compact(out[2])
    t = timed(lambda: K.compact(out[2], vpos))
    report("compact_flags", t, B, "flags", 1 + 8, "hbm")

    # ---------------- batch model + (a5) distance -------------------------
    S = 100
    from pyabc_amd.batch_models import LinearGaussianModel
    model = LinearGaussianModel.benchmark(d, S)
    theta = out[0]
    stats = model.simulate(theta, 1, 3, 0)
    t = timed(lambda: model.simulate(theta, 1, 3, 0))
    report("sim_linear_gaussian_f64", t, B, "proposals", 8 * d + 8 * S, "hbm",
           {"S": S})
    x0 = torch.as_tensor(model._x0, device="cuda")
    fw = torch.ones(S, dtype=F64, device="cuda")
    dd, acc, guard = K.pnorm_distance(stats, x0, fw, 2.0, 20.0)
    t = timed(lambda: K.pnorm_distance(stats, x0, fw, 2.0, 20.0, d_out=dd,
                                       acc_out=acc, guard_out=guard))
    report("pnorm_distance_f64", t, B, "particles", 8 * S + 10, "hbm",
           {"S": S})

    bench_sim_ode()

    # ------- (f3) exact inference: kernel density + stochastic acceptance --
    var = torch.full((S,), 0.25, dtype=F64, device="cuda")
    c = float(np.sum(np.log(2) + np.log(np.pi) + np.log(np.full(S, 0.25))))
    t = timed(lambda: K.stochastic_kernel(stats, x0, var, K.KERNEL_NORMAL, c,
                                          pdf_norm=-50.0, inv_temp=0.1,
                                          seed=1, stream=9))
    # stats 8S + pd 8 + accept 1 + weight 8 + guard 1 (u is in-kernel Philox)
    report("stochastic_kernel_accept_f64", t, B, "evaluations", 8 * S + 18,
           "hbm", {"S": S})
    pdv = dd.clone()
    lnum = torch.randn(B, dtype=F64, device="cuda", generator=g)
    lden = torch.randn(B, dtype=F64, device="cuda", generator=g)
    t = timed(lambda: K.tempered_sums(pdv, 30.0, [0.5], logw_num=lnum,
                                      logw_den=lden))
    report("tempered_sums_f64", t, B, "records", 24, "hbm", {"K": 1})

    # ---------------- (a6) adaptive scales --------------------------------
    for n in (200_000, 2_000_000 // q):
        data = stats[:, :n].contiguous() if n <= B else torch.randn(
            (S, n), dtype=F64, device="cuda", generator=g)
        t = timed(lambda: K.column_median_mad(data), reps=3)
        report("column_median_mad_f64", t, S * n, "values", 16, "hbm",
               {"S": S, "n": n})
        t = timed(lambda: K.column_std(data), reps=3)
        report("column_std_f64", t, S * n, "values", 8, "hbm",
               {"S": S, "n": n})

    # ---------------- (a4) normalisation + (a7) quantile -------------------
    dist = torch.rand(N, dtype=F64, device="cuda", generator=g)
    t = timed(lambda: K.dsum(w))
    report("sum_f64", t, N, "weights", 8, "hbm")
    t = timed(lambda: K.weighted_quantile(dist, w / w.sum(), 0.5))
    report("weighted_quantile_f64", t, N, "particles", 16, "hbm")

    # ---------------- (a8) LocalTransition (config 4) ----------------------
    N4, d4, k4 = 200_000 // q, 6, 50
    X4 = torch.randn((N4, d4), dtype=F64, device="cuda", generator=g)
    w4 = torch.rand(N4, dtype=F64, device="cuda", generator=g)
    w4 /= w4.sum()
    nbr, _ = K.knn(X4, k4)
    t = timed(lambda: K.knn(X4, k4), reps=2)
    report("knn_f64", t, N4 * N4, "pairs", 3 * d4, "valu_f32",
           {"N": N4, "d": d4, "k": k4})
    covs, invs, dets = K.local_cov(X4, w4, nbr)
    t = timed(lambda: K.local_cov(X4, w4, nbr))
    report("local_cov_f64", t, N4, "particles", 8 * (k4 * (d4 + 1) + 2 * d4 * d4 + 1)
           + 4 * k4, "hbm", {"N": N4, "d": d4, "k": k4})
    pts = X4 + 0.01
    t = timed(lambda: K.local_logpdf(pts, X4, w4, invs, dets), reps=2)
    report("local_logpdf_f64", t, N4 * N4, "pairs",
           3 * d4 + 2 * d4 * d4 + 4, "valu_f64", {"N": N4, "d": d4})
    t = timed(lambda: K.local_logpdf(pts, X4, w4, invs, dets, "f32"), reps=2)
    report("local_logpdf_f32", t, N4 * N4, "pairs",
           3 * d4 + 2 * d4 * d4 + 4, "valu_f32", {"N": N4, "d": d4})


if __name__ == "__main__":
    main()
