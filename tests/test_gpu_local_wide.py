"""LocalTransition at 9 to 16 parameters: the kNN fit, the exact fp64 density
and the matrix-core density (local_mfma16.hip) against plain numpy fp64, and
the public interface on top of them."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import ref_cpu as ref

pytestmark = pytest.mark.gpu

N, M, KNB = 300, 257, 40   # N no multiple of the 16-particle unit, M of 32


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pyabc_amd import kernels
    return kernels


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64,
                           device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def population(d, n):
    rng = np.random.default_rng(100 + d)
    X = rng.normal(size=(n, d)) * np.exp(rng.uniform(-1, 1, d)) + \
        rng.normal(size=d)
    w = rng.uniform(0.5, 1.5, n)
    return rng, X, w / w.sum()


@functools.lru_cache(maxsize=None)
def case(d):
    """Population, its numpy fit, and the rows: core (drawn from the
    transition), the same at 3 local sigmas, 8 of them at 40 local sigmas."""
    rng, X, w = population(d, N)
    covs, invs, dets = ref.local_covs(X, w, ref.knn_indices(X, KNB))
    idx = rng.integers(0, N, M)
    z = rng.normal(size=(M, d))
    L = np.linalg.cholesky(covs[idx])
    zn = z / np.linalg.norm(z, axis=1, keepdims=True)
    at = lambda zz: X[idx] + np.einsum("mab,mb->ma", L, zz)
    return dict(X=X, w=w, covs=covs, invs=invs, dets=dets, core=at(z),
                out3=at(zn * 3 * np.sqrt(d)), far=at(zn * 40)[:8])


def np_logpdf(c, pts):
    diff = pts[:, None, :] - c["X"][None, :, :]
    q = np.einsum("mna,nab,mnb->mn", diff, c["invs"], diff)
    d = c["X"].shape[1]
    e = np.log(c["w"]) - 0.5 * q - 0.5 * np.log((2 * np.pi) ** d * c["dets"])
    mx = e.max(axis=1, keepdims=True)
    return mx[:, 0] + np.log(np.exp(e - mx).sum(axis=1)) - np.log(c["w"].sum())


def logpdf(K, c, pts, prec, invs=None, dets=None, **kw):
    out = K.local_logpdf(dev(pts), dev(c["X"]), dev(c["w"]),
                         dev(c["invs"] if invs is None else invs),
                         dev(c["dets"] if dets is None else dets), prec, **kw)
    return (host(out[0]), out[1]) if kw else host(out)


@pytest.mark.parametrize("k", [20, 100])
@pytest.mark.parametrize("d", [9, 12, 16])
def test_knn(K, d, k):
    """Sets, order and fp64 distances of the all-fp64 scan (24 tiles, the
    last partial; both register forms), and a row range of it."""
    _, X, _ = population(d, 1500)
    want = ref.knn_indices(X, k)
    d2 = np.zeros(want.shape)
    for q in range(d):                  # the sequential sub / mul / add
        df = X[want, q] - X[:, None, q]
        d2 = d2 + df * df
    nbr, got = K.knn(dev(X), k)
    np.testing.assert_array_equal(host(nbr), want)
    np.testing.assert_array_equal(host(got), d2)
    nb, dd = K.knn_rows(dev(X), k, 700, 200)
    np.testing.assert_array_equal(host(nb), want[700:900])
    np.testing.assert_array_equal(host(dd), d2[700:900])


@pytest.mark.parametrize("d", [9, 12, 16])
def test_f64_density(K, d):
    """1e-12 relative on the density; the rows 40 sigmas out (density below
    the fp64 range) on the log."""
    c = case(d)
    pts = np.concatenate([c["core"], c["far"]])
    got, want = logpdf(K, c, pts, "f64"), np_logpdf(c, pts)
    err = np.abs(np.expm1(got[:M] - want[:M])).max()
    print(f"d={d} f64 max rel err {err:.3e}")
    assert err <= 1e-12
    np.testing.assert_allclose(got[M:], want[M:], rtol=1e-12)


@pytest.mark.parametrize("d", [9, 12, 16])
def test_mfma_density(K, d):
    """The matrix-core pass against the fp64 pass, 1e-5 relative, on rows
    from the transition and rows 3 local sigmas out; on the former it does
    the work itself (at most 5 of 257 rows in the fixup)."""
    c = case(d)
    got, nfix = logpdf(K, c, c["core"], "mfma", return_fixups=True)
    err = np.abs(np.expm1(got - logpdf(K, c, c["core"], "f64"))).max()
    got3 = logpdf(K, c, c["out3"], "mfma")
    err3 = np.abs(np.expm1(got3 - logpdf(K, c, c["out3"], "f64"))).max()
    print(f"d={d} mfma max rel err core {err:.3e} 3 sigma {err3:.3e} "
          f"fixups {nfix}")
    assert err <= 1e-5 and err3 <= 1e-5
    assert nfix <= 5


@pytest.mark.parametrize("d", [9, 12, 16])
def test_mfma_fixup_and_flag(K, d):
    """Rows 40 sigmas out take the exact fixup (the fp64 pass's bits, and
    counted); a particle whose Cholesky column norms span 2^20 sends every
    row through the fp64 pass."""
    c = case(d)
    pts = np.concatenate([c["core"], c["far"]])
    got, nfix = logpdf(K, c, pts, "mfma", return_fixups=True)
    exact = logpdf(K, c, pts, "f64")
    np.testing.assert_array_equal(got[M:], exact[M:])
    assert 8 <= nfix <= 8 + 5
    invs, dets = c["invs"].copy(), c["dets"].copy()
    invs[7] = np.diag([2.0 ** 40] + [1.0] * (d - 1))
    dets[7] = 2.0 ** -40
    np.testing.assert_array_equal(logpdf(K, c, pts, "mfma", invs, dets),
                                  logpdf(K, c, pts, "f64", invs, dets))


@pytest.mark.parametrize("d", [12, 16])
def test_mfma_launch_shape(K, d, monkeypatch):
    """A row's bits do not depend on the rows sharing its call nor on the
    launch-shape knobs."""
    c = case(d)
    base = logpdf(K, c, c["core"], "mfma")
    np.testing.assert_array_equal(logpdf(K, c, c["core"][:40], "mfma"),
                                  base[:40])
    for key, val in (("ABC_LZ_IB", "1"), ("ABC_LZ_TPB", "2")):
        monkeypatch.setenv(key, val)
        K.reload_tuning()
        got = logpdf(K, c, c["core"], "mfma")
        monkeypatch.delenv(key)
        K.reload_tuning()
        np.testing.assert_array_equal(got, base, err_msg=key)


@pytest.mark.parametrize("d", [10, 16])
def test_local_transition(K, d):
    import pyabc_amd as pa
    c = case(d)
    X, w, pts = c["X"], c["w"], c["core"][:64]
    cols = [f"p{q:02d}" for q in range(d)]
    tr = pa.LocalTransition(k=KNB, k_fraction=None)
    tr.fit(pd.DataFrame(X, columns=cols), w.copy())
    np.testing.assert_allclose(tr.covs, c["covs"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(tr.determinants, c["dets"], rtol=1e-12)
    np.testing.assert_allclose(
        tr.pdf(pd.DataFrame(pts, columns=cols)),
        ref.local_pdf(pts, X, w, c["invs"], c["dets"]), rtol=1e-5)
    draws = tr.rvs(1000)
    assert list(draws.columns) == cols and draws.shape == (1000, d)
    assert np.all(np.isfinite(draws.values))
    with pytest.raises(ValueError, match="mfma.*f64"):
        logpdf(K, c, pts, "f32")


def test_abcsmc_local_transition_d10(K):
    """Two generations of a 10-parameter linear-Gaussian model on the batch
    path with LocalTransition."""
    import pyabc_amd as pa
    d = 10
    A = np.random.RandomState(42).randn(30, d) / np.sqrt(d)
    x0 = A @ np.linspace(-1, 1, d) + 0.5 * np.random.RandomState(7).randn(30)
    keys = [f"y{k:03d}" for k in range(30)]
    names = [f"p{k:02d}" for k in range(d)]
    sampler = pa.GPUBatchSampler(seed=3)
    abc = pa.ABCSMC(pa.LinearGaussianModel(A, None, 0.5, keys=keys),
                    pa.Distribution(**{n: pa.RV("uniform", -5, 10) for n in names}),
                    pa.PNormDistance(p=2), population_size=2000,
                    transitions=pa.LocalTransition(k=50, k_fraction=None),
                    eps=pa.QuantileEpsilon(alpha=0.5), sampler=sampler)
    abc.new("mem://local_wide", dict(zip(keys, x0)))
    h = abc.run(max_nr_populations=2)
    assert all(e["batch"] for e in abc.generation_log), sampler.fallback_reason
    df, w = h.distribution_numpy(0, h.max_t)
    assert df[names].shape == (2000, d)
    np.testing.assert_allclose(w.sum(), 1.0, rtol=1e-9)
