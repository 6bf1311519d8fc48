"""MassActionODEModel: the device integrator against a high-precision scipy
reference on right-hand sides written out here, its batch-cut invariance, its
noise stream, the containment of a failing lane, and the model through
ABCSMC + GPUBatchSampler."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L10 = "log10theta"
_CHAIN = [f"A{i}" for i in range(1, 9)]


def _chain_rhs(x, th):
    flow = 10.0 ** th[0] * x[:-1] - 10.0 ** th[1] * x[1:]
    return np.append(-flow, 0.0) + np.append(0.0, flow)


# name -> (species, reactions, x_init, t_obs, observed, theta box lo, hi,
#          the right-hand side in numpy); k = 10 ** theta except in lv
NETS = {
    "conv": (["A", "B"],
             [({"A": 1}, {"B": 1}, (L10, 0)), ({"B": 1}, {"A": 1}, (L10, 1))],
             [1.0, 0.0], np.linspace(3, 30, 10), None, [-1, -1], [0.5, 0.5],
             lambda x, th: (10.0 ** th[1] * x[1] - 10.0 ** th[0] * x[0])
             * np.array([1.0, -1.0])),
    # constant rate: k2 = 0.3
    "dim": (["A", "B"],
            [({"A": 2}, {"B": 1}, (L10, 0)), ({"B": 1}, {"A": 2}, (L10, 1)),
             ({"B": 1}, {}, 0.3)],
            [1.0, 0.2], np.linspace(1, 10, 10), None, [-1, -1], [0.5, 0.5],
            lambda x, th: np.array([
                -2 * 10.0 ** th[0] * x[0] ** 2 + 2 * 10.0 ** th[1] * x[1],
                10.0 ** th[0] * x[0] ** 2 - 10.0 ** th[1] * x[1] - 0.3 * x[1]])),
    # I(0) from theta, two of three species observed
    "sir": (["S", "I", "R"],
            [({"S": 1, "I": 1}, {"I": 2}, (L10, 0)), ({"I": 1}, {"R": 1}, (L10, 1))],
            [0.99, ("theta", 2), 0.0], np.linspace(2, 20, 10), ["I", "R"],
            [-1, -1, 0.005], [0.5, 0.5, 0.02],
            lambda x, th: np.array([
                -10.0 ** th[0] * x[0] * x[1],
                10.0 ** th[0] * x[0] * x[1] - 10.0 ** th[1] * x[1],
                10.0 ** th[1] * x[1]])),
    "lv": (["X", "Y"],
           [({"X": 1}, {"X": 2}, ("theta", 0)),
            ({"X": 1, "Y": 1}, {"Y": 2}, ("theta", 1)),
            ({"Y": 1}, {}, ("theta", 2))],
           [1.0, 0.5], np.linspace(1.5, 15, 10), None, [0.5] * 3, [1.5] * 3,
           lambda x, th: np.array([th[0] * x[0] - th[1] * x[0] * x[1],
                                   th[1] * x[0] * x[1] - th[2] * x[1]])),
    # the largest instantiation: A1 <-> A2 <-> ... <-> A8, 14 reactions
    "chain8": (_CHAIN,
               [r for a, b in zip(_CHAIN, _CHAIN[1:])
                for r in (({a: 1}, {b: 1}, (L10, 0)), ({b: 1}, {a: 1}, (L10, 1)))],
               [1.0] + [0.0] * 7, np.linspace(1, 10, 10), None, [-1, -1],
               [0.5, 0.5], _chain_rhs),
}


def _model(pa, name, **kw):
    species, reactions, x_init, t_obs, observed = NETS[name][:5]
    return pa.MassActionODEModel(species, reactions, x_init, t_obs,
                                 observed=observed, **kw)


def _theta(name, B, seed=0):
    lo, hi = (np.asarray(v, dtype=float) for v in NETS[name][5:7])
    return lo + (hi - lo) * np.random.default_rng(seed).uniform(size=(B, lo.size))


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import pyabc_amd
    return pyabc_amd


def _dev(a):
    return torch.as_tensor(a, dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("name", list(NETS))
def test_accuracy_against_dop853(pa, name):
    """|device - DOP853(1e-13, 1e-15)| <= 50 (atol + rtol max_t |ref_s|) per
    proposal and species; scipy's own RK45 (the same pair and controller) is
    within 1.4 / 0.5 / 1.3 / 7.4 of these units on conv / dim / sir / lv and
    0.9 on chain8 ("Mass-action ODE model")."""
    from scipy.integrate import solve_ivp
    species, _, x_init, t_obs, observed, _, _, f = NETS[name]
    rtol, atol, B = 1e-8, 1e-11, 96   # two waves, the second part-filled
    theta = _theta(name, B)
    obs = [species.index(s) for s in (observed or species)]
    ref = np.empty((B, len(obs), t_obs.size))
    for b, th in enumerate(theta):
        x0 = [th[v[1]] if isinstance(v, tuple) else v for v in x_init]
        sol = solve_ivp(lambda t, x: f(x, th), (0, t_obs[-1]), x0, "DOP853",
                        t_eval=t_obs, rtol=1e-13, atol=1e-15)
        assert sol.success
        ref[b] = sol.y[obs]
    got = _model(pa, name, rtol=rtol, atol=atol).simulate(_dev(theta), 1, 2, 0)
    got = got.cpu().numpy().T.reshape(ref.shape)
    units = np.abs(got - ref) / (atol + rtol * np.abs(ref).max(2, keepdims=True))
    print(name, "worst error in units of atol + rtol max|ref|:", units.max())
    assert units.max() <= 50


def test_batch_cut_invariance(pa):
    """One call of 200 rows equals calls of 64, 1 and 135 rows at the matching
    offsets, bit for bit, noise included."""
    model = _model(pa, "lv", sigma=0.1)
    theta, off = _dev(_theta("lv", 200, seed=1)), 12345
    whole = model.simulate(theta, 7, 3, off)
    parts = [model.simulate(theta[a:b], 7, 3, off + a)
             for a, b in ((0, 64), (64, 65), (65, 200))]
    assert torch.equal(whole, torch.cat(parts, dim=1))


def test_noise_is_the_linear_gaussian_stream(pa):
    """simulate(sigma) - simulate(0) is sigma z of LinearGaussianModel's
    stream.  conv's statistics lie in [0.03, 1] and |sigma z| < 6e-3, so the
    noisy value is within a factor 1.2 of the clean one: its rounding error
    is at most one ulp of the clean value and the difference is exact."""
    from pyabc_amd import kernels as K
    sigma, seed, sid, off = 1e-3, 11, 5, 999
    theta = _dev(_theta("conv", 130, seed=2))
    clean = _model(pa, "conv").simulate(theta, seed, sid, off)
    noisy = _model(pa, "conv", sigma=sigma).simulate(theta, seed, sid, off)
    A = torch.zeros((clean.shape[0], 2), dtype=torch.float64, device="cuda")
    want = K.sim_linear_gaussian(theta, A, None, sigma, seed, sid, off)
    assert want.abs().max() > 0
    ulp = torch.as_tensor(np.spacing(clean.cpu().numpy()), device="cuda")
    assert torch.all((noisy - clean - want).abs() <= 2 * ulp)


def test_failing_lane_is_contained(pa):
    """A proposal that runs out of steps is a column of +inf, is rejected
    with a non-NaN distance, and leaves every other column as it was."""
    from pyabc_amd import kernels as K
    theta = _theta("lv", 96, seed=3)
    theta[5] *= 1e4
    theta = _dev(theta)
    short = _model(pa, "lv", max_steps=200).simulate(theta, 1, 2, 0)
    full = _model(pa, "lv").simulate(theta, 1, 2, 0)
    assert torch.all(short[:, 5] == np.inf)
    keep = torch.arange(96, device="cuda") != 5
    assert torch.isfinite(short[:, keep]).all()
    assert torch.equal(short[:, keep], full[:, keep])
    S = short.shape[0]
    d, acc, _ = K.pnorm_distance(short, _dev(np.ones(S)), _dev(np.ones(S)),
                                 2.0, 1e300)
    assert acc[5] == 0 and not torch.isnan(d[5]) and acc[keep].all()


@pytest.mark.parametrize("stochastic", [False, True])
def test_abcsmc_runs_on_the_device(pa, stochastic):
    """ABCSMC with the conversion reaction stays on the batch path; the
    stored statistics are simulate() of the stored parameters, bit for bit."""
    model = _model(pa, "conv")
    x0v = model.simulate(_dev([[-0.5, -0.3]]), 0, 0, 0)[:, 0].cpu().numpy()
    prior = pa.Distribution(k0=pa.RV("uniform", -1, 1.5),
                            k1=pa.RV("uniform", -1, 1.5))
    sampler = pa.GPUBatchSampler(seed=1)
    if stochastic:
        abc = pa.ABCSMC(model, prior, pa.IndependentNormalKernel(var=0.02 ** 2),
                        population_size=500, eps=pa.Temperature(),
                        acceptor=pa.StochasticAcceptor(), sampler=sampler)
    else:
        abc = pa.ABCSMC(model, prior, pa.PNormDistance(p=2),
                        population_size=2000, sampler=sampler)
    abc.new(pa.create_sqlite_db_id(), dict(zip(model.keys, x0v)))
    h = abc.run(max_nr_populations=2 if stochastic else 3)
    assert sampler.fallback_reason is None
    assert all(e["batch"] for e in abc.generation_log)
    if stochastic:
        return
    pops = h.get_all_populations()
    assert np.all(np.diff(pops[pops.t >= 0].epsilon.values) < 0)
    pop = h._pops[h.max_t]["population"]
    assert list(pop.stat_keys) == list(model.keys)
    assert torch.equal(pop.stats_T, model.simulate(pop.theta, 0, 0, 0))
