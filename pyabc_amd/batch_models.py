"""Batch simulators for the GPU sampler.

The reference evaluates one Python model call per proposal
(pyabc/model.py:92-123, 176-239).  The batch sampler instead asks a
:class:`BatchModel` for the statistics of B proposals at once, stat-major
``[S, B]`` on the device.  The two synthetic models below are the benchmark
models of BASELINE.json; each is one HIP kernel with
Philox4x32-10 noise.  :class:`MassActionODEModel` is the model class of the
reference's worked examples (doc/examples/conversion_reaction.ipynb,
noise.ipynb): a reaction-network ODE integrated per proposal by one kernel;
:class:`MassActionSSAModel` is the same network as a Markov jump process
(doc/examples/chemical_reaction.ipynb), simulated exactly per proposal.
"""
import numpy as np
import torch

from . import kernels as K


class BatchModel:
    """Interface: ``simulate(theta[B, d], seed, sid, offset) -> stats_T[S, B]``.

    ``keys`` are the summary-statistic names in x_0 order; ``name`` as in
    pyabc.Model.  ``offset`` is the global index of the first row, so that
    the noise of proposal i is the same however the batch is cut.
    """
    name = "batch_model"
    keys = ()

    @property
    def n_stats(self):
        return len(self.keys)

    def simulate(self, theta, seed, sid, offset):  # pragma: no cover
        raise NotImplementedError

    def observed(self):
        """x_0 as a dict in key order (optional)."""
        raise NotImplementedError


class LinearGaussianModel(BatchModel):
    """y = A theta + c + sigma * eps, eps ~ N(0, I_S)  (SURVEY C2/C5)."""

    def __init__(self, A, c=None, sigma=0.5, keys=None, name="linear_gaussian",
                 x0=None):
        A = np.asarray(A, dtype=np.float64)
        self.S, self.d = A.shape
        self.A_host = A
        self.c_host = None if c is None else np.asarray(c, dtype=np.float64)
        self.sigma = float(sigma)
        self.keys = tuple(keys) if keys is not None else tuple(
            f"y{k:03d}" for k in range(self.S))
        self.name = name
        self._x0 = x0
        self._dev = {}

    def _tensors(self):
        dev = torch.cuda.current_device()
        if dev not in self._dev:
            A = torch.as_tensor(self.A_host, device="cuda")
            c = None if self.c_host is None else torch.as_tensor(
                self.c_host, device="cuda")
            self._dev[dev] = (A, c)
        return self._dev[dev]

    def simulate(self, theta, seed, sid, offset):
        A, c = self._tensors()
        return K.sim_linear_gaussian(theta, A, c, self.sigma, seed, sid,
                                     offset)

    def simulate_distance(self, theta, seed, sid, offset, x0, fw, p, eps,
                          keep_stats=False):
        """simulate + p-norm distance + d <= eps in one pass (x0 / fw rows
        in the model's key order): (d, accept, guard), bit-identical to
        simulate() followed by the distance kernel; ``keep_stats``: the
        statistics simulate() returns as a fourth item, written by the same
        pass."""
        A, c = self._tensors()
        return K.sim_linear_gaussian_pnorm(theta, A, c, self.sigma, seed, sid,
                                           offset, x0, fw, p, eps,
                                           keep_stats=keep_stats)

    def simulate_host(self, theta, rng):
        """numpy reference of the same model (for CPU baselines)."""
        theta = np.atleast_2d(theta)
        y = theta @ self.A_host.T + self.sigma * rng.normal(
            size=(theta.shape[0], self.S))
        if self.c_host is not None:
            y = y + self.c_host
        return y

    def observed(self):
        return dict(zip(self.keys, self._x0))

    @staticmethod
    def benchmark(d, S=100, seed_A=42, seed_x0=7, sigma=0.5):
        """The synthetic inference problem of SURVEY 8(d): A =
        RandomState(42).randn(S,d)/sqrt(d), theta_true = linspace(-1,1,d),
        x_0 = A theta_true + sigma * RandomState(7).randn(S)."""
        A = np.random.RandomState(seed_A).randn(S, d) / np.sqrt(d)
        theta_true = np.linspace(-1, 1, d)
        x0 = A @ theta_true + sigma * np.random.RandomState(seed_x0).randn(S)
        m = LinearGaussianModel(A, None, sigma, x0=x0)
        m.theta_true = theta_true
        return m


class GaussianMeanModel(BatchModel):
    """Quickstart model: y = mean + 0.5 N(0,1)  (doc/examples/
    parameter_inference.ipynb, model cell)."""

    def __init__(self, sigma=0.5, key="data", name="model"):
        self.sigma = float(sigma)
        self.keys = (key,)
        self.name = name

    def simulate(self, theta, seed, sid, offset):
        out = K.sim_gaussian_mean(theta, self.sigma, seed, sid, offset)
        return out.view(1, -1)


class _MassActionNetwork(BatchModel):
    """What the mass-action models share: the network description, its
    validation and its compiled ``OdeTable``."""

    def _init_network(self, species, reactions, x_init, t_obs, observed,
                      keys, name, x0):
        from ._native import OdeTable
        self.species = tuple(species)
        n = len(self.species)
        if not 1 <= n <= OdeTable.MAX_SPECIES or len(set(self.species)) != n:
            raise ValueError(f"1 to {OdeTable.MAX_SPECIES} distinct species, "
                             f"got {self.species}")
        index = {s: i for i, s in enumerate(self.species)}

        def sp(name_):
            if name_ not in index:
                raise ValueError(f"unknown species {name_!r}")
            return index[name_]

        def counts(side):
            out = np.zeros(n, dtype=np.int64)
            for k, c in dict(side).items():
                if int(c) != c or c < 0:
                    raise ValueError(f"stoichiometry of {k!r} must be a "
                                     f"non-negative integer, got {c!r}")
                out[sp(k)] += int(c)
            return out

        def source(v, what, kinds):
            """(kind, theta column, constant) of a float or (kind, j)"""
            if isinstance(v, (tuple, list)):
                if len(v) != 2 or v[0] not in kinds or int(v[1]) != v[1] \
                        or not 0 <= v[1] < 32:
                    raise ValueError(f"{what}: expected a float or one of "
                                     f"{kinds} with a theta column, got {v!r}")
                return kinds.index(v[0]) + 1, int(v[1]), 0.0
            if not np.isfinite(float(v)):
                raise ValueError(f"{what}: {v!r} is not finite")
            return 0, -1, float(v)

        reactions = list(reactions)
        R = len(reactions)
        if not 1 <= R <= OdeTable.MAX_REACTIONS:
            raise ValueError(f"1 to {OdeTable.MAX_REACTIONS} reactions, got {R}")
        self.reactant_slots, self.net, self.rates = [], [], []
        for r, (lhs, rhs, rate) in enumerate(reactions):
            a, b = counts(lhs), counts(rhs)
            if a.sum() > 2:
                raise ValueError(f"reaction {r}: reactant order {a.sum()} > 2")
            slots = [i for i in range(n) for _ in range(a[i])]
            self.reactant_slots.append(tuple(slots + [-1] * (2 - len(slots))))
            self.net.append([(i, int(c)) for i, c in enumerate(b - a) if c])
            self.rates.append(source(rate, f"rate of reaction {r}",
                                     ("theta", "log10theta")))
        if isinstance(x_init, dict):
            for k in x_init:
                sp(k)
            x_init = [x_init.get(s, 0.0) for s in self.species]
        if len(x_init) != n:
            raise ValueError(f"x_init has {len(x_init)} entries for {n} species")
        self.x_init = [source(v, f"x_init of {s}", ("theta",))
                       for s, v in zip(self.species, x_init)]
        self.t_obs = np.atleast_1d(np.asarray(t_obs, dtype=np.float64))
        T = self.t_obs.size
        if self.t_obs.ndim != 1 or T < 1 or not np.all(np.isfinite(self.t_obs)) \
                or self.t_obs[0] <= 0 or np.any(np.diff(self.t_obs) <= 0):
            raise ValueError("t_obs must be positive and strictly increasing")
        self.observed_species = tuple(self.species if observed is None
                                      else observed)
        obs = [sp(s) for s in self.observed_species]
        if not obs or len(set(obs)) != len(obs):
            raise ValueError("observed must name distinct species")
        self.S = T * len(obs)
        if self.S > OdeTable.MAX_STATS:
            raise ValueError(f"S = T * len(observed) = {self.S} > "
                             f"{OdeTable.MAX_STATS}")
        self.keys = tuple(keys) if keys is not None else tuple(
            f"{s}_{j:03d}" for s in self.observed_species for j in range(T))
        if len(self.keys) != self.S:
            raise ValueError(f"{len(self.keys)} keys for {self.S} statistics")
        self.name = name
        self._x0 = x0
        # theta columns the network reads: theta must have more than this
        self.max_col = max(c for _, c, _ in self.rates + self.x_init)

        tab = self.table = OdeTable()
        tab.n_species, tab.n_reactions = n, R
        tab.n_times, tab.n_observed = T, len(obs)
        p = 0
        for r in range(R):
            tab.rate_kind[r], tab.rate_col[r], tab.rate_const[r] = self.rates[r]
            tab.reactant[r][0], tab.reactant[r][1] = self.reactant_slots[r]
            tab.pair_start[r] = p
            for i, c in self.net[r]:
                tab.pair[p] = (c << 8) | i
                p += 1
        tab.pair_start[R] = p
        for i, (_, col, const) in enumerate(self.x_init):
            tab.x_init_col[i], tab.x_init[i] = col, const
        for o, i in enumerate(obs):
            tab.observed[o] = i
        tab.t_obs[:T] = self.t_obs.tolist()

    def _check_theta(self, d):
        if not self.max_col < d <= 32:
            raise ValueError(f"the network reads theta column {self.max_col}; "
                             f"theta has {d} columns (at most 32)")

    def observed(self):
        x0 = self._x0
        return x0 if isinstance(x0, dict) or x0 is None else dict(
            zip(self.keys, x0))


class MassActionODEModel(_MassActionNetwork):
    """Mass-action kinetics ``dx/dt = sum_r nu_r k_r prod(reactants of r)``
    observed at fixed times, integrated on the device with an adaptive
    Dormand-Prince 5(4) pair (scipy ``RK45``'s controller), one lane per
    proposal.

    ``species``: 1 to 8 names.  ``reactions``: 1 to 16 entries ``(reactants,
    products, rate)``; reactants and products are dicts ``name -> count``
    (non-negative integers, at most two reactant molecules: ``{}``, ``{A: 1}``,
    ``{A: 1, B: 1}``, ``{A: 2}``; the propensity of ``2A ->`` is ``k A A``);
    ``rate`` is a float, ``("theta", j)`` (column j of theta) or
    ``("log10theta", j)`` (``10 ** theta_j``).  ``x_init``: per species (a
    sequence in species order, or a dict by name, missing names starting at
    0) a float or ``("theta", j)``.
    ``t_obs``: strictly increasing positive times; ``observed``: the observed
    species (default all).

    Statistics: species blocks in ``observed`` order, time-major within a
    block -- statistic ``o * T + j`` is observed species o at ``t_obs[j]``,
    default key ``f"{species}_{j:03d}"``; ``S = T * len(observed) <= 256``.
    With ``sigma > 0`` the noise is :class:`LinearGaussianModel`'s (the same
    Philox stream and fast normals).  A proposal whose integration needs more
    than ``max_steps`` attempted steps or stops being finite has ``+inf`` in
    every statistic, so it is rejected and never a NaN.
    """

    def __init__(self, species, reactions, x_init, t_obs, observed=None,
                 sigma=0.0, rtol=1e-6, atol=1e-9, max_steps=100000, keys=None,
                 name="mass_action_ode", x0=None):
        self._init_network(species, reactions, x_init, t_obs, observed, keys,
                           name, x0)
        if not (rtol > 0 and atol >= 0 and max_steps >= 1):
            raise ValueError("rtol > 0, atol >= 0 and max_steps >= 1")
        self.sigma, self.rtol, self.atol = float(sigma), float(rtol), float(atol)
        self.max_steps = int(max_steps)

    def simulate(self, theta, seed, sid, offset):
        self._check_theta(theta.shape[1])
        return K.sim_mass_action_ode(theta, self.table, self.rtol, self.atol,
                                     self.max_steps, self.sigma, seed, sid,
                                     offset)

    def simulate_host(self, theta, rng=None):
        """scipy statement of the same model (for CPU baselines): RK45 at the
        model's tolerances, [B, S]; noise needs ``rng`` when sigma > 0."""
        from scipy.integrate import solve_ivp
        theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
        self._check_theta(theta.shape[1])
        n, R = len(self.species), len(self.rates)
        nu = np.zeros((n, R))
        for r, pairs in enumerate(self.net):
            for i, c in pairs:
                nu[i, r] = c
        slots = np.array(self.reactant_slots)
        obs = [self.species.index(s) for s in self.observed_species]
        out = np.empty((theta.shape[0], self.S))
        for b, th in enumerate(theta):
            k = np.array([c if kind == 0 else th[col] if kind == 1
                          else 10.0 ** th[col] for kind, col, c in self.rates])
            x0 = np.array([c if kind == 0 else th[col]
                           for kind, col, c in self.x_init])

            def f(t, x):
                xe = np.append(x, 1.0)      # slot -1 reads the trailing 1
                return nu @ (k * xe[slots[:, 0]] * xe[slots[:, 1]])
            sol = solve_ivp(f, (0.0, self.t_obs[-1]), x0, method="RK45",
                            t_eval=self.t_obs, rtol=self.rtol, atol=self.atol)
            out[b] = sol.y[obs].ravel() if sol.success else np.inf
        if self.sigma > 0:
            out = out + self.sigma * rng.normal(size=out.shape)
        return out


class MassActionSSAModel(_MassActionNetwork):
    """The Markov jump process of a mass-action network on integer molecule
    counts, observed at fixed times and simulated exactly on the device with
    Gillespie's direct method, one lane per proposal (the model class of the
    reference's doc/examples/chemical_reaction.ipynb).

    The network description, the statistic layout ``o * T + j`` and the
    default keys are :class:`MassActionODEModel`'s.  What differs: the state
    is integer counts; a constant ``x_init`` entry must be a non-negative
    integer and a ``("theta", j)`` one is ``rint(theta_j)``; the propensity of
    ``2A ->`` is ``k x_A (x_A - 1)``, the ordered-pair convention, whose
    large-count limit is the ODE model's ``k A A``; and there is no ``sigma``:
    observation noise is what ``BinomialKernel`` / ``PoissonKernel`` /
    ``NegativeBinomialKernel`` model.  include/abc_hip.h states the process
    and its random-number stream; :meth:`simulate_host` restates it in numpy.

    A proposal with a negative or non-finite rate, an initial count from
    theta outside ``[0, 2^31)``, a count leaving that range, or more than
    ``max_events`` (1 to 2^24) events before the last observation time has
    ``+inf`` in every statistic: a p-norm distance rejects it, never a NaN.
    ``kernels.count_kernel`` answers a ``+inf`` statistic as scipy's logpmf
    does, with a NaN density, and its fused acceptance (``NaN >= u`` is
    false) rejects the proposal.
    """

    def __init__(self, species, reactions, x_init, t_obs, observed=None,
                 max_events=1 << 20, keys=None, name="mass_action_ssa",
                 x0=None):
        self._init_network(species, reactions, x_init, t_obs, observed, keys,
                           name, x0)
        for s, (kind, _, c) in zip(self.species, self.x_init):
            if kind == 0 and not (0 <= c < 2 ** 31 and c == int(c)):
                raise ValueError(f"x_init of {s}: a molecule count must be an "
                                 f"integer in [0, 2^31), got {c!r}")
        if int(max_events) != max_events or not 1 <= max_events <= 1 << 24:
            raise ValueError("1 <= max_events <= 2^24")
        self.max_events = int(max_events)

    def simulate(self, theta, seed, sid, offset, events_out=None):
        self._check_theta(theta.shape[1])
        return K.sim_mass_action_ssa(theta, self.table, self.max_events, seed,
                                     sid, offset, events_out=events_out)

    def simulate_host(self, theta, u, info=False, tie_tol=1e-9):
        """The same process in numpy on caller-supplied uniforms: ``u[b]``
        holds ``(u1, u2)`` of event e of row b at ``[2 e, 2 e + 1]``.  The
        propensities and their sums are fp64 in the device's order; event
        times are carried in ``numpy.longdouble``.  Returns ``[B, S]``; with
        ``info`` also the events fired per row and whether the row came
        within a relative ``tie_tol`` of a tie (an event time against an
        observation time, or ``u2 a0`` against a running sum), where one
        rounding could change the path."""
        theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
        u = np.atleast_2d(np.asarray(u, dtype=np.float64))
        self._check_theta(theta.shape[1])
        T, obs = self.t_obs.size, [self.species.index(s)
                                   for s in self.observed_species]
        out = np.empty((theta.shape[0], self.S))
        events = np.zeros(theta.shape[0], dtype=np.int64)
        tie = np.zeros(theta.shape[0], dtype=bool)
        for b, th in enumerate(theta):
            k = np.array([c if kind == 0 else th[col] if kind == 1
                          else 10.0 ** th[col] for kind, col, c in self.rates])
            x = np.array([c if kind == 0 else np.rint(th[col])
                          for kind, col, c in self.x_init])
            stats = np.full((len(obs), T), np.inf)
            ok = np.all((k >= 0) & (k < np.inf)) and \
                np.all((x >= 0) & (x < 2.0 ** 31))
            x = x.astype(np.int64) if ok else x
            t, j, e = np.longdouble(0), 0, 0
            while ok:
                a = np.empty(len(k))
                for r, (sa, sb) in enumerate(self.reactant_slots):
                    v = k[r]
                    if sa >= 0:
                        v = v * np.float64(x[sa])
                    if sb >= 0:
                        v = v * np.float64(x[sb] - (sb == sa))
                    a[r] = v
                run = np.cumsum(a)      # sequential fp64 adds
                a0 = run[-1]
                if a0 == 0:
                    stats[:, j:] = x[obs][:, None]
                    break
                if 2 * e + 1 >= u.shape[1]:
                    raise ValueError(f"row {b} needs more than {e} events' "
                                     f"uniforms")
                u1, u2 = u[b, 2 * e], u[b, 2 * e + 1]
                tn = t + np.longdouble(-np.log(1.0 - u1) / a0)
                tie[b] |= bool(np.any(
                    np.abs(self.t_obs[j:] - tn) <= tie_tol * self.t_obs[j:]))
                while j < T and self.t_obs[j] < tn:
                    stats[:, j] = x[obs]
                    j += 1
                if j == T:
                    break
                target = u2 * a0
                tie[b] |= bool(np.any(np.abs(run[a > 0] - target)
                                      <= tie_tol * a0))
                hit = np.flatnonzero(run > target)
                r = hit[0] if hit.size else np.flatnonzero(a > 0)[-1]
                for i, c in self.net[r]:
                    x[i] += c
                t, e = tn, e + 1
                if x.min() < 0 or x.max() >= 2 ** 31 or e >= self.max_events:
                    stats[:] = np.inf
                    break
            out[b], events[b] = stats.ravel(), e
        return (out, events, tie) if info else out


def _per_particle_accept(model, t, pars, sum_stats_calculator,
                         distance_calculator, eps_calculator, acceptor, x_0):
    """One proposal through a batch model (closure sampling path): B = 1 on
    the device, then the acceptor, as Model.accept does (model.py:176-239)."""
    from .model import ModelResult
    res = model.summary_statistics(t, pars, sum_stats_calculator)
    acc = acceptor(distance_function=distance_calculator, eps=eps_calculator,
                   x=res.sum_stats, x_0=x_0, t=t, par=pars)
    res.distance = acc.distance
    res.accepted = acc.accept
    res.weight = acc.weight
    return res


def _per_particle_stats(model, t, pars, sum_stats_calculator):
    from .model import ModelResult
    names = sorted(pars.keys())
    theta = torch.as_tensor(np.array([[float(pars[k]) for k in names]]),
                            device="cuda")
    seed = int(np.random.randint(0, 2 ** 62, dtype=np.int64))
    stats = model.simulate(theta, seed, 0, 0)[:, 0].cpu().numpy()
    return ModelResult(sum_stats=sum_stats_calculator(
        dict(zip(model.keys, stats))))


BatchModel.summary_statistics = _per_particle_stats
BatchModel.accept = _per_particle_accept
