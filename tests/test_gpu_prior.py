"""The device prior table (prior.hip): density against mpmath, the support
flag against scipy's pdf > 0, inversion draws against scipy's ppf of the same
uniforms, rejection draws against scipy's cdf, cut invariance, and ABCSMC on
the batch path with priors that are not a uniform box."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# family -> (shapes, interior z range of the density test)
FAMS = {"uniform": ((), (1e-3, 0.999)), "norm": ((), (-6, 6)),
        "lognorm": ((0.7,), (1e-3, 20)), "expon": ((), (0, 30)),
        "laplace": ((), (-20, 20)), "loguniform": ((0.01, 100.0), (0.011, 99)),
        "truncnorm": ((-1.5, 4.0), (-1.499, 3.999)),
        "gamma": ((2.5,), (1e-3, 30)), "beta": ((0.5, 2.0), (1e-3, 0.999))}
LOC, SCALE = 1.5, 2.0


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pyabc_amd
    return pyabc_amd


def _dev(a):
    return torch.as_tensor(a, dtype=torch.float64, device="cuda")


def _prior(pa, specs):
    """specs: [(family, shapes, loc, scale)] -> (table, frozen scipy rvs)."""
    rvs = {f"p{i:02d}": pa.RV(f, *sh, loc=loc, scale=sc)
           for i, (f, sh, loc, sc) in enumerate(specs)}
    names, table = pa.Distribution(**rvs).device_table()
    return table, [rvs[n].distribution for n in names]


def _mp_terms(fam, sh, z, scale):
    """The family's log density at z, term by term, at 50 digits."""
    import mpmath as mp
    mp.mp.dps = 50
    z, sh, L = mp.mpf(float(z)), [mp.mpf(s) for s in sh], mp.log
    half_l2pi = L(2 * mp.pi) / 2
    return {"uniform": lambda: [],
            "norm": lambda: [-z * z / 2, -half_l2pi],
            "lognorm": lambda: [-L(z), -L(z) ** 2 / (2 * sh[0] ** 2),
                                -L(sh[0]) - half_l2pi],
            "expon": lambda: [-z],
            "laplace": lambda: [-abs(z), -L(2)],
            "loguniform": lambda: [-L(z), -L(L(sh[1]) - L(sh[0]))],
            "truncnorm": lambda: [-z * z / 2, -half_l2pi,
                                  -L(mp.ncdf(sh[1]) - mp.ncdf(sh[0]))],
            "gamma": lambda: [(sh[0] - 1) * L(z), -z, -mp.loggamma(sh[0])],
            "beta": lambda: [(sh[0] - 1) * L(z), (sh[1] - 1) * L(1 - z),
                             mp.loggamma(sh[0] + sh[1]) - mp.loggamma(sh[0])
                             - mp.loggamma(sh[1])],
            }[fam]() + [-L(mp.mpf(scale))]


@pytest.mark.parametrize("fams", [(f,) for f in FAMS] + [
    ("lognorm", "beta", "norm"), ("gamma", "uniform", "truncnorm"),
    ("laplace", "loguniform", "expon")])
def test_density_against_mpmath(pa, fams):
    """|logp - ref| <= 1e-12 (1 + sum |terms| + sum |constants|), pd = exp of
    it to the same relative 1e-12; one full tile and a ragged one."""
    import mpmath as mp
    from pyabc_amd import kernels as K
    B = 257 if len(fams) == 1 else 1000
    table, _ = _prior(pa, [(f, FAMS[f][0], LOC, SCALE) for f in fams])
    rng = np.random.default_rng(len(fams[0]))
    theta = np.stack([LOC + SCALE * rng.uniform(*FAMS[f][1], size=B)
                      for f in fams], axis=1)
    z = (theta - LOC) / SCALE
    logp, pd, sup = K.prior_logpdf(_dev(theta), table)
    logp, pd = logp.cpu().numpy(), pd.cpu().numpy()
    assert sup.all()
    worst = 0.0
    for b in range(B):
        terms = [t for k, f in enumerate(fams)
                 for t in _mp_terms(f, FAMS[f][0], z[b, k], SCALE)]
        ref, size = mp.fsum(terms), 1 + mp.fsum(abs(t) for t in terms)
        worst = max(worst, float(abs(logp[b] - ref) / size),
                    float(abs(pd[b] / mp.exp(ref) - 1)))
    print(f"{fams}: worst error / bound unit {worst:.2e}")
    assert worst <= 1e-12


SUPPORT = [(f, sh) for f, (sh, _) in FAMS.items()] + [
    ("gamma", (0.5,)), ("gamma", (1.0,)), ("beta", (2.0, 0.5)),
    ("beta", (2.0, 5.0)), ("beta", (0.5, 0.5)), ("beta", (1.0, 1.0))]


@pytest.mark.parametrize("loc,scale", [(-3.0, 0.5), (LOC, SCALE)])
@pytest.mark.parametrize("fam,sh", SUPPORT)
def test_support_is_scipy_pdf_positive(pa, fam, sh, loc, scale):
    """The ends of the support, an ulp either side, NaN and +-inf.  loc != 0,
    so the neighbours of an end at z = 0 are z ~ 1e-16: with loc = 0 they are
    the subnormal 5e-324, where scipy's own beta pdf raises OverflowError."""
    from pyabc_amd import kernels as K
    table, (rv,) = _prior(pa, [(fam, sh, loc, scale)])
    ends = [loc + scale * e for e in rv.dist.support(*sh) if np.isfinite(e)]
    theta = np.array([v for e in ends for v in (
        np.nextafter(e, -np.inf), e, np.nextafter(e, np.inf))]
        + [np.nan, np.inf, -np.inf, loc + 0.5 * scale])
    logp, pd, sup = (t.cpu().numpy() for t in
                     K.prior_logpdf(_dev(theta[:, None]), table))
    with np.errstate(all="ignore"):
        want = rv.pdf(theta) > 0
    assert np.array_equal(sup.astype(bool), want), (theta, sup, want)
    assert not np.isnan(logp).any() and not np.isnan(pd).any()
    # -inf outside the interval; inside it a density that underflows keeps
    # its true (very negative) logarithm
    assert np.all(pd[~want] == 0) and np.all(np.exp(logp[~want]) == 0)


INVERSION = [("uniform", ()), ("norm", ()), ("lognorm", (0.7,)), ("expon", ()),
             ("laplace", ()), ("loguniform", (0.01, 100.0)),
             ("truncnorm", (-1.5, 4.0)), ("truncnorm", (1.0, 5.0))]


def test_inversion_draws_against_scipy_ppf(pa):
    from pyabc_amd import kernels as K
    seed, sid, off, B, d = 11, 6, 77, 1000, len(INVERSION)
    table, rvs = _prior(pa, [(f, sh, LOC, SCALE) for f, sh in INVERSION])
    theta = K.prior_rvs(table, d, seed, sid, off, B)
    u = K.philox_uniform(seed, sid, off * d, B * d).view(B, d).cpu().numpy()
    got = theta.cpu().numpy()
    for k, rv in enumerate(rvs):
        ref = rv.ppf(u[:, k])
        err = np.max(np.abs(got[:, k] - ref) / (np.abs(ref - LOC) + SCALE))
        print(f"{INVERSION[k]}: {err:.2e}")
        assert err <= 1e-12, INVERSION[k]
    box = K.prior_uniform(_dev(np.full(d, LOC)), _dev(np.full(d, SCALE)), seed,
                          sid, off, B)
    assert torch.equal(theta[:, 0], box[:, 0])


@pytest.mark.parametrize("fam,sh", [("gamma", (0.5,)), ("gamma", (3.0,)),
                                    ("beta", (0.5, 2.0)), ("beta", (2.0, 5.0))])
def test_rejection_draws_against_scipy_cdf(pa, fam, sh):
    """Kolmogorov distance within the DKW bound at alpha = 1e-9."""
    from pyabc_amd import kernels as K
    n = 1 << 17
    table, (rv,) = _prior(pa, [(fam, sh, LOC, SCALE)])
    x = np.sort(K.prior_rvs(table, 1, 5, 2, 0, n).view(-1).cpu().numpy())
    assert not np.isnan(x).any()
    F, i = rv.cdf(x), np.arange(n)
    dist = max(np.max(np.abs((i + 1) / n - F)), np.max(np.abs(i / n - F)))
    print(f"{fam}{sh}: D = {dist:.4f}")
    assert dist <= np.sqrt(np.log(2 / 1e-9) / (2 * n))


def test_draws_do_not_depend_on_the_cut(pa):
    from pyabc_amd import kernels as K
    table, _ = _prior(pa, [(f, sh, LOC, SCALE) for f, (sh, _) in FAMS.items()])
    d, B, B1, off = len(FAMS), 300, 131, 5
    whole = K.prior_rvs(table, d, 3, 4, off, B)
    parts = torch.cat([K.prior_rvs(table, d, 3, 4, off, B1),
                       K.prior_rvs(table, d, 3, 4, off + B1, B - B1)])
    assert torch.equal(whole, parts) and not torch.isnan(whole).any()


@pytest.mark.parametrize("case", ["norm", "mixed"])
def test_abcsmc_with_a_table_prior(pa, case):
    """Three generations on the batch path; the last generation's weights are
    prior.pdf / transition.pdf recomputed on the host in fp64 (1e-5: the KDE
    pass's contract), and every accepted particle lies in the support."""
    from oracle import ref_cpu as ref
    if case == "norm":
        model = pa.GaussianMeanModel()
        prior = pa.Distribution(mu=pa.RV("norm", 0, 2))
        x0 = {"data": 1.0}
    else:
        model = pa.LinearGaussianModel(np.array([[1.0, 0.5], [0.0, 2.0]]),
                                       sigma=0.3)
        prior = pa.Distribution(a=pa.RV("lognorm", 0.8),
                                b=pa.RV("beta", 0.7, 1.5))
        x0 = dict(zip(model.keys, [0.4, 0.2]))
    sampler = pa.GPUBatchSampler(seed=7)
    abc = pa.ABCSMC(model, prior, pa.PNormDistance(p=2), population_size=2000,
                    sampler=sampler)
    abc.new(pa.create_sqlite_db_id(), x0)
    h = abc.run(max_nr_populations=3)
    assert sampler.fallback_reason is None
    assert all(e["batch"] for e in abc.generation_log)
    (Xp, wp), (X, w) = (h.distribution_numpy(0, t)
                        for t in (h.max_t - 1, h.max_t))
    names = sorted(prior)
    Xp, X = Xp[names].values, X[names].values
    ppd = np.prod([prior[n].pdf(X[:, k]) for k, n in enumerate(names)], axis=0)
    assert np.all(ppd > 0)
    want = ppd / ref.kde_transition_pd(X, Xp, wp, ref.mvn_fit_cov(Xp, wp))
    want /= want.sum()
    err = np.max(np.abs(np.asarray(w) / want - 1))
    print(f"{case}: weights max rel err {err:.2e}")
    assert err <= 1e-5
