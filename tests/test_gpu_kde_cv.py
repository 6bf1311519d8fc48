"""GridSearchCV on the device: the cross-validation kernel (kde_cv.hip)
against a longdouble reference, run-to-run determinism, the class and an
ABCSMC run.  Tolerances are the project's fp32 density contract (README:
1e-5 relative on a density = 1e-5 absolute on its logarithm)."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

LD = np.longdouble
# (n, d, k, G): smallest; leave-one-out; padded d, odd G, folds inside tiles;
# past 16 dimensions; two row tiles per fold, four column segments of one
# chunk each (one empty) and a grid above the 8 values of one launch; blocks
# that walk two chunks (32 segments over 34) and three (22 over 45): the
# double-buffered hand-over and the in-loop rescale of the running sum
SHAPES = [(7, 1, 3, 1), (9, 2, 9, 2), (131, 5, 5, 7), (300, 17, 4, 5),
          (200, 3, 3, 9), (2400, 2, 10, 3), (5700, 1, 2, 1)]
CASES = [s + ("plain",) for s in SHAPES] + [
    (131, 5, 5, 7, "decades"), (131, 5, 5, 7, "far"),
    (2400, 2, 10, 3, "decades"), (2400, 2, 10, 3, "far")]


@functools.lru_cache(maxsize=None)
def reference(n, d, k, G, variant="plain", seed=3):
    """Seeded inputs and, per fold, np.cov(aweights) * silverman^2, its eigh
    whitening and the longdouble log-sum-exp over the training rows."""
    from pyabc_amd.transition import kfold_offsets, silverman_rule_of_thumb
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)) * rng.uniform(0.5, 2.0, d) + 1.0
    w = rng.uniform(0.5, 1.5, n)
    if variant == "decades":
        w = 10.0 ** rng.uniform(-30, 0, n)
    if variant == "far":
        X[n // 2] += 50.0 * X.std(0)
    w /= w.sum()
    grid = np.linspace(0.05, 1.0, G)
    off = kfold_offsets(n, k)
    L = np.empty((G, n), LD)
    c = np.empty((k, G), LD)
    mu, Us = np.empty((k, d)), np.empty((k, d, d))
    for f in range(k):
        te, tr = np.arange(off[f], off[f + 1]), np.r_[0:off[f], off[f + 1]:n]
        cov = np.atleast_2d(np.cov(X[tr].T, aweights=w[tr])) * \
            silverman_rule_of_thumb(1 / (w[tr] ** 2).sum(), d) ** 2
        s, u = np.linalg.eigh(cov)
        mu[f], Us[f] = np.average(X[tr], axis=0, weights=w[tr]), u / np.sqrt(s)
        z = X.astype(LD) @ Us[f].astype(LD)
        q = ((z[te][:, None, :] - z[tr][None]) ** 2).sum(-1)
        for g, sc in enumerate(grid):
            e = np.log(w[tr].astype(LD))[None] - q / (2 * LD(sc))
            m = e.max(1, keepdims=True)
            L[g, te] = m[:, 0] + np.log(np.exp(e - m).sum(1))
            c[f, g] = -(d * np.log(2 * LD(np.pi)) + np.log(s.astype(LD)).sum()
                        + d * np.log(LD(sc))) / 2
    score = np.array([[(w[off[f]:off[f + 1]] * L[g, off[f]:off[f + 1]]).sum()
                       for g in range(G)] for f in range(k)])
    return dict(X=X, w=w, grid=grid, off=off, mu=mu, Us=Us, L=L, c=c,
                score=score)


def score_tol(r, score_ref):
    wabs = np.add.reduceat(np.abs(r["w"]), r["off"][:-1])
    return 1e-5 * wabs[:, None] + 1e-12 * np.abs(score_ref).astype(float)


def run_kernel(r):
    from pyabc_amd import kernels as K
    dv = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda")
    L, score = K.kde_cv(dv(r["X"]), dv(r["w"]), r["off"], dv(r["mu"]),
                        dv(r["Us"]), r["grid"])
    return L.cpu().numpy(), score.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_kernel_against_longdouble(case):
    r = reference(*case)
    L, score = run_kernel(r)
    assert np.isfinite(r["L"]).all() and np.isfinite(L).all()
    err = np.abs(L - r["L"]).max()
    serr = (np.abs(score - r["score"]) / score_tol(r, r["score"])).max()
    print(f"kde_cv {case}: max |L - L_ref| = {float(err):.3e}, "
          f"score error / tolerance = {float(serr):.3e}")
    assert err <= 1e-5
    assert serr <= 1.0


def test_bit_equal_between_calls():
    r = reference(2400, 2, 10, 3)
    a, b = run_kernel(r), run_kernel(r)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_class_selects_the_reference_scaling():
    import pyabc_amd as pa
    r = reference(131, 5, 5, 7)
    full = np.asarray((r["score"] + r["c"] * np.add.reduceat(
        r["w"], r["off"][:-1])[:, None]), dtype=float)
    mean_ref, tol = full.mean(0), score_tol(r, full).mean(0)
    top = np.sort(mean_ref)[::-1]
    assert top[0] - top[1] > 2 * tol.max()     # the seed's margin (CPU fact)
    df = pd.DataFrame(r["X"], columns=[f"p{j}" for j in range(5)])
    gs = pa.GridSearchCV(param_grid={"scaling": r["grid"]}).fit(df, r["w"].copy())
    got = gs.cv_results_["mean_test_score"]
    print("GridSearchCV mean score error / tolerance:",
          (np.abs(got - mean_ref) / tol).max())
    assert (np.abs(got - mean_ref) <= tol).all()
    best = r["grid"][int(np.argmax(mean_ref))]
    assert gs.best_params_ == {"scaling": best}
    assert not any("train" in key for key in gs.cv_results_)
    plain = pa.MultivariateNormalTransition(scaling=best)
    plain.fit(df, r["w"].copy())
    np.testing.assert_array_equal(gs.pdf(df), plain.pdf(df))
    # any other estimator: the generic host loop
    loc = pa.GridSearchCV(estimator=pa.LocalTransition(k=20),
                          param_grid={"scaling": [0.5, 1.0]}).fit(
                              df, r["w"].copy())
    assert np.isfinite(loc.cv_results_["mean_test_score"]).all()
    assert isinstance(loc.best_estimator_, pa.LocalTransition)


def test_abcsmc_with_gridsearch_on_the_batch_path():
    import pyabc_amd as pa
    from tests.conftest import load_golden
    g = load_golden("e2e_stats")
    np.random.seed(0)
    sampler = pa.GPUBatchSampler(seed=11)
    abc = pa.ABCSMC(pa.GaussianMeanModel(),
                    pa.Distribution(mean=pa.RV("uniform", 0, 5)),
                    pa.PNormDistance(p=2), population_size=500,
                    eps=pa.MedianEpsilon(), transitions=pa.GridSearchCV(),
                    sampler=sampler)
    abc.new("mem://gridsearch", {"data": 2.5})
    h = abc.run(minimum_epsilon=0.05, max_nr_populations=3)
    assert sampler.fallback_reason is None
    assert all(e["batch"] for e in abc.generation_log)
    assert "scaling" in abc.transitions[0].best_params_
    df, w = h.distribution_numpy(0, h.max_t)
    mean = float((df["mean"].values * w).sum() / w.sum())
    # the band of test_gpu_api's C1 check, at this run's last generation
    ref_mean = np.array([g[f"c1_mean_{r}"][h.max_t] for r in range(5)])
    ref_std = np.array([g[f"c1_std_{r}"][h.max_t] for r in range(5)])
    spread = ref_mean.std() + ref_std.mean() / np.sqrt(200)
    assert abs(mean - ref_mean.mean()) < 5 * spread + 1e-3
