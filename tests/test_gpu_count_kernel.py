"""Binomial / Poisson / NegativeBinomial kernels on the device
(``abc_count_kernel_f64``) against mpmath at 50 digits and scipy.

Bound: |pd - ref| <= (K_TERM + S) 2^-53 mag, mag the sum of the absolute
terms; K_TERM = 4.5 is derived in DESIGN.md and must stay below four times
scipy's own worst error on the same inputs (1.40, 6.78, 1.80 in 2^-53 mag).
Measured max err / bound on an MI355X: 0.074 (binomial), 0.094 (Poisson),
0.085 (negative binomial)."""
import functools

import mpmath as mp
import numpy as np
import pytest
import scipy.stats
import torch

pytestmark = pytest.mark.gpu

mp.mp.dps = 50
EPS = 2.0 ** -53
K_TERM = 4.5
T = 4096
BINOM, POISSON, NEGBIN = 3, 4, 5
SCIPY = {BINOM: lambda k, n, p: scipy.stats.binom.logpmf(k=k, n=n, p=p),
         POISSON: lambda k, n, p: scipy.stats.poisson.logpmf(k=k, mu=n),
         NEGBIN: lambda k, n, p: scipy.stats.nbinom.logpmf(k=k, n=n, p=p)}
SHAPES = [(1, 1, 1), (3, 65, 72), (130, 67, 67),
          (770, 2, 2)]   # past one LDS chunk of 768 statistics
KIND_P = [(BINOM, 0.03), (BINOM, 0.5), (BINOM, 0.97), (POISSON, None),
          (NEGBIN, 0.03), (NEGBIN, 0.5), (NEGBIN, 0.97)]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pyabc_amd import kernels
    return kernels


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def lf(m):
    return mp.loggamma(m + 1)


def reference(kind, k, N, p):
    """mpmath log-pmf sum and sum of |terms| per column of the integers N"""
    lp, l1p = (mp.log(p), mp.log1p(-p)) if p is not None else (None, None)
    ref, mag = [], []
    for col in N.T:
        tot = big = mp.mpf(0)
        for ks, n in zip(k.tolist(), col.tolist()):
            if kind == BINOM:
                ts = [lf(n), -lf(ks), -lf(n - ks), ks * lp, (n - ks) * l1p]
            elif kind == POISSON:
                ts = [ks * mp.log(n) if ks else mp.mpf(0), -mp.mpf(n), -lf(ks)]
            else:
                ts = [lf(ks + n - 1), -lf(ks), -lf(n - 1), n * lp, ks * l1p]
            tot += mp.fsum(ts)
            big += mp.fsum(abs(t) for t in ts)
        ref.append(tot)
        mag.append(big)
    return ref, mag


def ratio(got, ref, mag, S):
    """max |got - ref| / ((K_TERM + S) 2^-53 mag)"""
    return max(float(abs(mp.mpf(float(g)) - r) / ((K_TERM + S) * EPS * m))
               for g, r, m in zip(got, ref, mag))


@functools.lru_cache(maxsize=None)
def problem(kind, S, B, ld, p):
    """Seeded counts: columns 0..63 (the first wave) keep every log-factorial
    argument well below T; later columns cycle through T-1, T, T+1 (n - k
    straddling T, n above it), 1e6, 2^40 and small values.  The one-element
    problem has k >= T, n near 1e6.  Padding columns B..ld are NaN."""
    rng = np.random.default_rng([kind, S, B])
    k = rng.integers(0, 50, size=S)
    N = k[:, None] + rng.integers(1, 2000, size=(S, B))
    cls = rng.integers(0, 6, size=(S, B))
    edge = np.choose(cls, [N, T - 1 + k[:, None] * (N % 2), T + k[:, None] * (N % 2),
                           T + 1 + k[:, None] * (N % 2), 10 ** 6 + N, 2 ** 40 + N])
    N[:, 64:] = edge[:, 64:]
    if B == 1:
        k[:], N[:] = 5000, 10 ** 6 + 7
    full = np.full((S, ld), np.nan)
    full[:, :B] = N + rng.uniform(0, 0.9, size=N.shape)   # truncated away
    x0 = k + rng.uniform(0, 0.9, size=S)
    return (full, x0, k, N) + reference(kind, k, N, p)


def test_table(K):
    tab = host(K.count_table())
    for row, f in ((tab[0], lambda m: lf(m)), (tab[1][1:], lambda m: mp.log(m + 1))):
        want = [f(m) for m in range(len(row))]
        err = [abs(mp.mpf(float(v)) - w) for v, w in zip(row, want)]
        assert all(e <= np.spacing(abs(float(w))) for e, w in zip(err, want))


@pytest.mark.parametrize("kind", [BINOM, POISSON, NEGBIN])
def test_k_term_within_four_times_scipy(kind):
    worst = 0.0
    for p in [q for kd, q in KIND_P if kd == kind]:
        for S, B, ld in SHAPES:
            _, _, k, N, ref, mag = problem(kind, S, B, ld, p)
            sc = SCIPY[kind](k[:, None], N, p).sum(0)
            worst = max(worst, ratio(sc, ref, mag, S) * (K_TERM + S))
    print("scipy worst err / (2^-53 mag)", worst)
    assert K_TERM <= 4 * worst


@pytest.mark.parametrize("S,B,ld", SHAPES)
@pytest.mark.parametrize("kind,p", KIND_P)
def test_kernel_against_mpmath(K, kind, p, S, B, ld):
    full, x0, k, N, ref, mag = problem(kind, S, B, ld, p)
    pd, _, _, _ = K.count_kernel(dev(full)[:, :B], dev(x0), p, kind)
    r = ratio(host(pd), ref, mag, S)
    print("max err / bound", r)
    assert r <= 1.0


@pytest.mark.parametrize("kind,k,n,p", [
    (BINOM, 6, 5, 0.3), (BINOM, -1, 5, 0.3), (BINOM, 0, 0, 0.3),
    (BINOM, 0, -1, 0.3), (BINOM, -1, -1, 0.3), (BINOM, 0, 5, 0.0),
    (BINOM, 2, 5, 0.0), (BINOM, 5, 5, 1.0), (BINOM, 2, 5, 1.0),
    (BINOM, 0, 0, 1.0), (BINOM, 2, np.inf, 0.3), (BINOM, 2, np.nan, 0.3),
    (BINOM, 2, 2.0 ** 52, 0.3),
    (POISSON, 0, 0, None), (POISSON, 2, 0, None), (POISSON, -1, 3, None),
    (POISSON, 0, -1, None), (POISSON, -1, -1, None), (POISSON, 2, -np.inf, None),
    (NEGBIN, 0, 0, 0.5), (NEGBIN, 0, -2, 0.5), (NEGBIN, -1, -2, 0.5),
    (NEGBIN, -1, 3, 0.5), (NEGBIN, 0, 5, 1.0), (NEGBIN, 3, 5, 1.0),
    (NEGBIN, 0, 5, 0.0), (NEGBIN, 3, 5, 0.0), (NEGBIN, 3, np.nan, 0.5),
])
def test_edge_semantics(K, kind, k, n, p):
    """Every row is out of support or exactly 0 in scipy; a statistic that is
    not finite or is >= 2^52 has no integer value and gives NaN."""
    want = SCIPY[kind](k, int(n), p) if abs(n) < 2.0 ** 52 else np.nan
    assert not np.isfinite(want) or want == 0.0
    pd, _, _, _ = K.count_kernel(dev([[n]]), dev([k]), p, kind)
    np.testing.assert_array_equal(host(pd), [want])


@pytest.mark.parametrize("kind,p", [(BINOM, 0.5), (POISSON, None), (NEGBIN, 0.03)])
def test_position_independence_and_fused_acceptance(K, kind, p):
    S, B, ld = 130, 67, 67
    full, x0, _, _, ref, _ = problem(kind, S, B, ld, p)
    wide = np.full((S, 80), np.nan)
    wide[:, :B] = full
    st, x0d = dev(wide), dev(x0)
    kw = dict(pdf_norm=float(max(ref)), inv_temp=1e-3, seed=5, stream=3)
    whole = K.count_kernel(st[:, :B], x0d, p, kind, offset=100, **kw)
    lo = K.count_kernel(st[:, :37], x0d, p, kind, offset=100, **kw)
    hi = K.count_kernel(st[:, 37:B], x0d, p, kind, offset=137, **kw)
    packed = K.count_kernel(dev(full[:, 37:B]), x0d, p, kind, offset=137, **kw)
    for w, a, b, q in zip(whole, lo, hi, packed):
        np.testing.assert_array_equal(host(w), np.concatenate([host(a), host(b)]))
        np.testing.assert_array_equal(host(b), host(q))      # ld 80 vs 30
    assert 0 < host(whole[1]).sum() < B
    u = dev(np.random.default_rng(2).uniform(size=B))
    for iw in (True, False):
        pd, acc, accw, guard = K.count_kernel(
            st[:, :B], x0d, p, kind, pdf_norm=kw["pdf_norm"], inv_temp=1e-3,
            apply_iw=iw, u=u)
        np.testing.assert_array_equal(host(pd), host(whole[0]))
        want = K.stochastic_accept(pd, kw["pdf_norm"], 1e-3, apply_iw=iw, u=u)
        for got, w in zip((acc, accw, guard), want):
            np.testing.assert_array_equal(host(got), host(w))
    # grid cap 1024 blocks x 256: B = 3920 * 67 = 1024 * 256 + 496 gives block
    # 0 a full second grid-stride pass and block 1 a ragged one (240 columns)
    pd, _, _, _ = K.count_kernel(dev(full).repeat(1, 3920), x0d, p, kind)
    np.testing.assert_array_equal(host(pd).reshape(3920, B),
                                  np.broadcast_to(host(whole[0]), (3920, B)))


@pytest.mark.parametrize("name,p", [("BinomialKernel", 0.3), ("PoissonKernel", None),
                                    ("NegativeBinomialKernel", 0.3)])
def test_classes(K, name, p):
    import pyabc_amd as pa
    cls, S, B, args = getattr(pa, name), 3, 50, () if p is None else (p,)
    full, x0v, k, N, ref, mag = problem(cls._kind, 3, 65, 72, p)
    keys = [f"s{i}" for i in range(S)]
    x0, kern = dict(zip(keys, x0v)), cls(*args)
    kern.initialize(0, None, x0)
    assert kern.batch_unsupported_reason(x0) is None
    pd, _, _ = kern.batch(dev(full[:, :B]), 0, x0)
    one = [kern(dict(zip(keys, full[:, b])), x0) for b in range(B)]
    assert ratio(host(pd) - np.array(one), [mp.mpf(0)] * B, mag[:B], S) <= 1.0
    bad = [(cls(*args, ret_scale=pa.SCALE_LIN), x0),
           (cls(*args), {"s0": np.array([3.0, 4.0])})]
    bad += [(cls(lambda par: p), x0)] if p is not None else []
    for kern, obs in bad:
        kern.initialize(0, None, obs)
        assert kern.batch_unsupported_reason(obs) is not None


@pytest.mark.parametrize("name,p", [("PoissonKernel", None), ("BinomialKernel", 0.3)])
def test_e2e_count_kernel_batch_path(K, name, p):
    """No fallback and stored distances that are scipy's; for Poisson also
    temperature 1 and the posterior mean of a host quadrature."""
    import pyabc_amd as pa
    cls, S = getattr(pa, name), 8
    kind = cls._kind
    A = np.linspace(0.6, 5.5, S)[:, None]
    c = np.full(S, 5.0)                      # trunc(A theta + c) in [5, 60]
    scale = 1.0 if p is None else 1.0 / p    # binomial: n ~ k / p
    kobs = np.trunc((A[:, 0] * 4.0 + c) / scale) + np.array([1, -2, 0, 3, -1, 2, -3, 1])
    keys = [f"y{s:02d}" for s in range(S)]
    sampler = pa.GPUBatchSampler(seed=77)
    abc = pa.ABCSMC(pa.LinearGaussianModel(A, c, sigma=0.0, keys=keys),
                    pa.Distribution(p0=pa.RV("uniform", 0, 10)),
                    cls(*(() if p is None else (p,))), population_size=2000,
                    eps=pa.Temperature(), acceptor=pa.StochasticAcceptor(),
                    sampler=sampler)
    abc.new(pa.create_sqlite_db_id(), dict(zip(keys, kobs)))
    h = abc.run(max_nr_populations=6)
    assert sampler.fallback_reason is None
    got = h.get_population(h.max_t).get_for_keys(["distance", "sum_stat"])
    N = np.array([[st[key] for key in keys] for st in got["sum_stat"]]).astype(int).T
    k, (_, mag) = kobs.astype(int), reference(kind, kobs.astype(int), N, p)
    sc = SCIPY[kind](k[:, None], N, p).sum(0)
    assert ratio(np.array(got["distance"]) - sc, [mp.mpf(0)] * len(sc), mag, S) <= 1.0
    if p is not None:
        return
    assert h.get_all_populations().query("t >= 0").epsilon.values[-1] == 1.0
    grid = (np.arange(400000) + 0.5) / 40000
    like = np.exp(scipy.stats.poisson.logpmf(
        k[:, None], np.trunc(A * grid[None, :] + c[:, None])).sum(0))
    mean = (grid * like).sum() / like.sum()
    std = np.sqrt(((grid - mean) ** 2 * like).sum() / like.sum())
    df, w = h.distribution_numpy(0, h.max_t)
    x, w = df["p0"].values, w / w.sum()
    assert abs((x * w).sum() - mean) < 5 * std / np.sqrt(1 / np.sum(w ** 2))
