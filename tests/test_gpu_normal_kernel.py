"""Full-covariance NormalKernel on the device (``abc_normal_kernel_f64``, fp64
MFMA): the kernel against the same formula in ``np.longdouble`` under a
derived rounding bound, the class against the reference's golden densities,
position independence and the fused acceptance bitwise, and a
StochasticAcceptor + Temperature run against the analytic posterior."""
import numpy as np
import pytest
import torch

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


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


def _problem(S, R, B, ld, seed=0):
    """Seeded inputs (dense non-symmetric U, diffs of order 1; the padding
    columns B..ld are NaN) and the longdouble reference with its bound."""
    rng = np.random.default_rng([seed, S, R, B])
    full = np.full((S, ld), np.nan)
    full[:, :B] = rng.normal(size=(S, B)) + 3.0
    x0 = rng.normal(size=S) + 3.0
    U = rng.normal(size=(S, R)) / np.sqrt(S)
    c = 1.2345 * S - 7.0
    ld_ = np.longdouble
    diff = full[:, :B].astype(ld_) - x0.astype(ld_)[:, None]
    y = diff.T @ U.astype(ld_)
    ref = -0.5 * (ld_(c) + (y * y).sum(1))
    A = ((np.abs(diff).T @ np.abs(U).astype(ld_)) ** 2).sum(1)
    bound = 2 * (0.5 * (2 * S + R + 3) * EPS * A + 2 * EPS * np.abs(ref))
    return full, x0, U, c, ref, bound


@pytest.mark.parametrize("S,R,B,ld", [
    (1, 1, 1, 1),          # smallest shape
    (5, 2, 16, 16),        # one full tile, ld == B, asymmetric U
    (3, 3, 17, 24),        # column tail
    (17, 17, 67, 80),      # k-tail, r-tail, second wave and block tail
    (131, 130, 70, 70),    # past one r-block of 128 and an LDS chunk of 16
])
def test_kernel_against_longdouble(K, S, R, B, ld):
    full, x0, U, c, ref, bound = _problem(S, R, B, ld)
    pd, acc, accw, guard = K.normal_kernel(dev(full)[:, :B], dev(x0), dev(U), c)
    assert acc is None and accw is None and guard is None
    err = np.abs(host(pd).astype(np.longdouble) - ref)
    print("max err / bound", float(np.max(err / bound)))
    assert np.all(err <= bound)


def test_class_matches_reference_golden(K):
    import pyabc_amd as pa
    g = load_golden("stoch_kernel_full")
    keys = [f"s{i}" for i in range(g["X"].shape[1])]
    x0 = dict(zip(keys, g["x0"]))
    k = pa.NormalKernel(cov=g["cov"])
    k.initialize(0, None, x0)
    assert k.batch_unsupported_reason(x0) is None
    pd, _, _ = k.batch(dev(g["X"].T), 0, x0)
    np.testing.assert_allclose(host(pd), g["normal_full_log"], rtol=1e-12)
    lin = pa.NormalKernel(cov=g["cov"], ret_scale=pa.SCALE_LIN)
    lin.initialize(0, None, x0)
    assert lin.batch_unsupported_reason(x0) is not None


def test_position_independence_and_fused_acceptance(K):
    S, R, B, ld = 17, 17, 67, 80
    full, x0, U, c, ref, _ = _problem(S, R, B, ld, seed=1)
    st, x0d, Ud = dev(full), dev(x0), dev(U)
    kw = dict(pdf_norm=float(ref.max()), inv_temp=0.2, seed=5, stream=3)
    whole = K.normal_kernel(st[:, :B], x0d, Ud, c, offset=100, **kw)
    lo = K.normal_kernel(st[:, :37], x0d, Ud, c, offset=100, **kw)
    hi = K.normal_kernel(st[:, 37:B], x0d, Ud, c, offset=137, **kw)
    packed = K.normal_kernel(dev(full[:, 37:B]), x0d, Ud, c, offset=137, **kw)
    for w, a, b, p in zip(whole, lo, hi, packed):
        np.testing.assert_array_equal(host(w), np.concatenate([host(a), host(b)]))
        np.testing.assert_array_equal(host(b), host(p))      # ld 80 vs 30
    assert 0 < host(whole[1]).sum() < B
    # injected uniforms: the decision is stochastic_accept of the kernel's pd
    u = dev(np.random.default_rng(2).uniform(size=B))
    for iw in (True, False):
        pd, acc, accw, guard = K.normal_kernel(
            st[:, :B], x0d, Ud, c, pdf_norm=kw["pdf_norm"], inv_temp=0.2,
            apply_iw=iw, u=u)
        np.testing.assert_array_equal(host(pd), host(whole[0]))
        want = K.stochastic_accept(pd, kw["pdf_norm"], 0.2, apply_iw=iw, u=u)
        for got, w in zip((acc, accw, guard), want):
            np.testing.assert_array_equal(host(got), host(w))


def test_e2e_normal_kernel_batch_path(K):
    """ABCSMC + NormalKernel(cov) + StochasticAcceptor through the GPU batch
    sampler: no fallback, final temperature 1, analytic posterior (precision
    A' C^-1 A) within Monte-Carlo error."""
    import pyabc_amd as pa
    g = load_golden("e2e_stochastic")
    A, x0v, var = g["A"], g["x0"], float(g["var"])
    S, d = A.shape
    L = np.eye(S) + 0.3 * np.tril(np.random.default_rng(11).normal(size=(S, S)), -1)
    C = var * L @ L.T                      # cond ~ 18; posterior well inside
    Ci = np.linalg.inv(C)                  # the prior box
    cov = np.linalg.inv(A.T @ Ci @ A)
    mean, std = cov @ (A.T @ Ci @ x0v), np.sqrt(np.diag(cov))
    keys = [f"y{k:02d}" for k in range(S)]
    names = [f"p{k}" for k in range(d)]
    sampler = pa.GPUBatchSampler(seed=2025)
    abc = pa.ABCSMC(pa.LinearGaussianModel(A, sigma=0.0, keys=keys),
                    pa.Distribution(**{n: pa.RV("uniform", -5, 10) for n in names}),
                    pa.NormalKernel(cov=C), population_size=4000,
                    eps=pa.Temperature(), acceptor=pa.StochasticAcceptor(),
                    sampler=sampler)
    abc.new(pa.create_sqlite_db_id(), dict(zip(keys, x0v)))
    h = abc.run(max_nr_populations=6)
    assert sampler.fallback_reason is None
    pops = h.get_all_populations()
    assert pops[pops.t >= 0].epsilon.values[-1] == 1.0
    df, w = h.distribution_numpy(0, h.max_t)
    X, w = df[names].values, w / w.sum()
    m = (X * w[:, None]).sum(0)
    s = np.sqrt(((X - m) ** 2 * w[:, None]).sum(0))
    ess = 1 / np.sum(w ** 2)
    assert np.all(np.abs(m - mean) < 5 * std / np.sqrt(ess)), (m, mean)
    np.testing.assert_allclose(s, std, rtol=0.1)
