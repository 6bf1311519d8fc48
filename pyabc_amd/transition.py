"""GPU-backed transitions with the reference's plug-in API.

Reference: pyabc/transition/base.py:13-123 (Transition), transitionmeta.py:
7-51 (no-parameter handling and fit-weight normalisation),
multivariatenormal.py:42-125 (MultivariateNormalTransition),
local_transition.py:13-145 (LocalTransition) and model_selection.py:9-69
(GridSearchCV).  fit / rvs / pdf compute through
the HIP kernels (weighted moments, Philox proposals, KDE pass; kNN, local
covariances, local density); only d x d factorisations run on the host, where
the reference also calls numpy/scipy on d x d matrices.
"""
import copy
import functools
import math
from abc import ABCMeta, abstractmethod

import numpy as np
import pandas as pd
import torch

from . import kernels as K
from .distributed import Comm
from .engine import (DeviceMVNFit, _side_stream, start_cdf,
                     silverman_rule_of_thumb,
                     scott_rule_of_thumb)
from .frames import DeviceFrame, as_device_matrix, as_device_vector

__all__ = ["Transition", "DiscreteTransition", "MultivariateNormalTransition",
           "LocalTransition", "GridSearchCV", "kfold_offsets",
           "NotEnoughParticles", "silverman_rule_of_thumb",
           "scott_rule_of_thumb"]


class NotEnoughParticles(Exception):
    pass


def _ncols(X):
    return len(X.columns) if hasattr(X, "columns") else np.shape(X)[1]


def _wrap_fit(f):
    @functools.wraps(f)
    def fit(self, X, w):
        self.X = X
        self.w = w
        if _ncols(X) == 0:
            self.no_parameters = True
            return
        self.no_parameters = False
        if isinstance(w, torch.Tensor):
            if w.numel() > 0:
                s = float(K.dsum(as_device_vector(w)).item())
                if not np.isclose(s, 1):
                    w = w / s
                    self.w = w
        elif np.size(w) > 0:
            if not np.isclose(w.sum(), 1):
                w /= w.sum()
        f(self, X, w)
    return fit


def _wrap_pdf(f):
    @functools.wraps(f)
    def pdf(self, x):
        if self.no_parameters:
            return 1
        return f(self, x)
    return pdf


def _wrap_rvs_single(f):
    @functools.wraps(f)
    def rvs_single(self):
        if self.no_parameters:
            return pd.Series(dtype=float)
        return f(self)
    return rvs_single


class TransitionMeta(ABCMeta):
    """Wraps fit/pdf/rvs_single for the zero-parameter case and normalises
    the fit weights (transitionmeta.py:7-51)."""

    def __init__(cls, name, bases, attrs):
        ABCMeta.__init__(cls, name, bases, attrs)
        if "fit" in attrs:
            cls.fit = _wrap_fit(attrs["fit"])
        if "pdf" in attrs:
            cls.pdf = _wrap_pdf(attrs["pdf"])
        if "rvs_single" in attrs:
            cls.rvs_single = _wrap_rvs_single(attrs["rvs_single"])


class Transition(metaclass=TransitionMeta):
    NR_BOOTSTRAP = 5
    X = None
    w = None
    no_parameters = False

    @abstractmethod
    def fit(self, X, w):
        """Fit to the weighted population ``X`` (DataFrame / DeviceFrame)."""

    @abstractmethod
    def rvs_single(self):
        """One sample as a pd.Series indexed by the parameter names."""

    def rvs(self, size=None):
        if size is None:
            return self.rvs_single()
        return pd.DataFrame([self.rvs_single() for _ in range(size)])

    @abstractmethod
    def pdf(self, x):
        """Density at a Series (-> float) or DataFrame (-> ndarray)."""

    def score(self, X, w):
        return (np.log(self.pdf(X)) * w).sum()

    def no_meaningful_particles(self):
        return len(self.X) == 0 or self.no_parameters

    def get_params(self, deep=True):
        return {}

    def set_params(self, **params):
        for k, v in params.items():
            setattr(self, k, v)
        return self


class DiscreteTransition(Transition):
    """Base class of discrete transition kernels."""


def _columns(X):
    return list(X.columns)


def _draw_seed():
    # the reference draws from numpy's global RandomState; seeding it with
    # np.random.seed therefore also fixes the device Philox streams here
    return int(np.random.randint(0, 2 ** 62, dtype=np.int64))


def _as_output(arr, single, columns):
    if single:
        return pd.Series(arr[0], index=columns)
    return pd.DataFrame(arr, columns=columns)


class MultivariateNormalTransition(Transition):
    """Gaussian KDE perturbation kernel on the GPU.

    fit: weighted moments kernel + host d x d finish (smart_cov * bw^2 *
    scaling, multivariatenormal.py:67-85).  rvs: device resampling +
    perturbation (Philox).  pdf: device KDE pass (exact-grid f16 MFMA by
    default; ``kde_precision="f32"`` for the direct fp32 kernel,
    ``kde_precision="f64"`` for the fp64 kernel).
    """

    def __init__(self, scaling=1, bandwidth_selector=silverman_rule_of_thumb,
                 kde_precision="mfma"):
        self.scaling = scaling
        self.bandwidth_selector = bandwidth_selector
        self.kde_precision = kde_precision
        self._fit = None

    def fit(self, X, w):
        if len(X) == 0:
            raise NotEnoughParticles("Fitting not possible.")
        Xd, _ = as_device_matrix(X)
        wd = as_device_vector(w)
        if Xd.is_cuda:
            # the resampling CDF and the KDE pack on the side stream,
            # overlapping the host's d x d finish (engine.start_cdf)
            c = start_cdf(wd)
            self._fit = DeviceMVNFit(Xd, wd, self.scaling,
                                     self.bandwidth_selector,
                                     self.kde_precision,
                                     pack_stream=_side_stream())
            self._fit.adopt_cdf(*c)
        else:
            self._fit = DeviceMVNFit(Xd, wd, self.scaling,
                                     self.bandwidth_selector,
                                     self.kde_precision)
        self.cov = self._fit.cov

    # device-level API used by the batch sampler
    @property
    def device_fit(self):
        return self._fit

    def rvs(self, size=None):
        if size is None:
            return self.rvs_single()
        return self._draw(size, single=False)

    def rvs_single(self):
        return self._draw(1, single=True)

    def _draw(self, size, single):
        f = self._fit
        theta, _, _ = K.propose_philox(f.X, f.cdf, f.A, None, None,
                                       _draw_seed(), 0, 0, size)
        return _as_output(theta.cpu().numpy(), single, _columns(self.X))

    def pdf(self, x):
        single = isinstance(x, pd.Series) or (
            not isinstance(x, (pd.DataFrame, DeviceFrame, torch.Tensor))
            and np.ndim(x) == 1)
        theta, _ = as_device_matrix(x, columns=_columns(self.X)
                                    if isinstance(x, (pd.Series, pd.DataFrame,
                                                      DeviceFrame)) else None)
        dens = torch.exp(self._fit.logpdf(theta)).cpu().numpy()
        if single or dens.size == 1:
            return float(dens[0])
        return dens

    def logpdf_device(self, theta, parent=None):
        """log density at device rows; ``parent`` (optional): per row an
        index into the fitted population (kde_mfma.hip per-row offsets;
        the density does not depend on it)."""
        return self._fit.logpdf(theta, parent)


class LocalTransition(Transition):
    """Local (k-nearest-neighbour covariance) Gaussian kernel on the GPU
    (local_transition.py:13-145): kNN by the one-pass device top-k, per
    particle weighted covariance + LU det/inverse, density by the device
    quadratic-form pass.  Up to 16 parameters; the fp32 pair loop
    ``kde_precision="f32"`` serves up to 8 (above, "mfma" is the 1e-5 path
    and the first density call with "f32" raises)."""
    EPS = 1e-3
    MIN_K = 10

    def __init__(self, k=None, k_fraction=1 / 4, scaling=1,
                 kde_precision="mfma"):
        # kde_precision: the density pass as the z form on the f16 matrix
        # cores "mfma" (the default: 1e-5 relative, measured 1.4e-6 at C4;
        # 21.5 vs 35.1 ms for "f32" at N = M = 2e5, d = 6), the fp32 pair
        # loop "f32" (1e-5) or "f64" (1e-12)
        if kde_precision not in ("f32", "f64", "mfma"):
            raise ValueError(f"unknown kde_precision {kde_precision!r}")
        self.kde_precision = kde_precision
        if k_fraction is not None:
            self.k_fraction = k_fraction
            self._k = None
        else:
            self.k_fraction = None
            self._k = k
        self.scaling = scaling

    @property
    def k(self):
        if self.k_fraction is not None:
            k_ = 0 if self.w is None else int(self.k_fraction * len(self.w))
        else:
            k_ = self._k
        try:
            dim = self._Xd.shape[1]
        except AttributeError:
            dim = 0
        return max([k_, self.MIN_K, dim])

    def fit(self, X, w):
        if len(X) == 0:
            raise NotEnoughParticles("Fitting not possible.")
        self._Xd, _ = as_device_matrix(X)
        self._wd = as_device_vector(w)
        n, d = self._Xd.shape
        kk = min(self.k + 1, n) - 1          # query(k+1) minus self
        if kk == 0:
            # single particle: deltas = |X|, one unit weight (:126-128)
            x0 = self._Xd[0].cpu().numpy()
            c = np.diag(np.abs(x0))
            if np.abs(c.sum()) == 0:
                c = np.diag(np.abs(x0))
            c = c * self.scaling
            det = np.linalg.det(c)
            while det <= 0:
                c += np.identity(d) * self.EPS
                det = np.linalg.det(c)
            covs = torch.as_tensor(c[None], device=self._Xd.device)
            invs = torch.as_tensor(np.linalg.inv(c)[None],
                                   device=self._Xd.device)
            dets = torch.as_tensor([det], device=self._Xd.device)
        else:
            comm = Comm.current()
            if comm.active:
                # each rank fits its row share, one all-gather
                # of (covs, inverses, dets); every row equals the 1-rank fit
                q, m = divmod(n, comm.world)
                r = comm.rank
                lo = r * q + min(r, m)
                hi = lo + q + (1 if r < m else 0)
                sizes = [q + (1 if s < m else 0) for s in range(comm.world)]
                nbr, _ = K.knn_rows(self._Xd, kk, lo, hi - lo)
                c, i, dt = K.local_cov_rows(self._Xd, self._wd, nbr, lo,
                                            self.scaling)
                packed = torch.cat([c.reshape(hi - lo, -1),
                                    i.reshape(hi - lo, -1),
                                    dt.view(-1, 1)], 1)
                allp = comm.all_gather_rows(packed, sizes)
                covs = allp[:, :d * d].reshape(n, d, d).contiguous()
                invs = allp[:, d * d:2 * d * d].reshape(n, d, d).contiguous()
                dets = allp[:, 2 * d * d].contiguous()
                nbr = comm.all_gather_rows(nbr.to(torch.int64), sizes).to(
                    torch.int32)
            else:
                nbr, _ = K.knn(self._Xd, kk)
                covs, invs, dets = K.local_cov(self._Xd, self._wd, nbr,
                                               self.scaling)
            self.nbr = nbr
        self._covs, self._invs, self._dets = covs, invs, dets
        self._cdf = K.resample_cdf(self._wd)

    # device-level API used by the batch sampler (engine.GenerationEngine)
    @property
    def device_fit(self):
        if getattr(self, "_covs", None) is None:
            return None
        return _LocalDeviceFit(self)

    @property
    def covs(self):
        return self._covs.cpu().numpy()

    @property
    def inv_covs(self):
        return self._invs.cpu().numpy()

    @property
    def determinants(self):
        return self._dets.cpu().numpy()

    @property
    def normalization(self):
        d = self._Xd.shape[1]
        return np.sqrt((2 * np.pi) ** d * self.determinants)

    @property
    def X_arr(self):
        return self._Xd.cpu().numpy()

    def pdf(self, x):
        single = isinstance(x, pd.Series)
        theta, _ = as_device_matrix(x, columns=_columns(self.X)
                                    if isinstance(x, (pd.Series, pd.DataFrame,
                                                      DeviceFrame)) else None)
        dens = torch.exp(self.logpdf_device(theta)).cpu().numpy()
        if single:
            return float(dens[0])
        return dens

    def logpdf_device(self, theta, parent=None):
        return K.local_logpdf(theta, self._Xd, self._wd, self._invs,
                              self._dets, self.kde_precision)

    def rvs_single(self):
        return self._draw(1, True)

    def rvs(self, size=None):
        if size is None:
            return self.rvs_single()
        return self._draw(size, False)

    def _draw(self, size, single):
        theta, _, _ = K.propose_local(self._Xd, self._cdf, self._covs,
                                      _draw_seed(), 0, 0, size)
        return _as_output(theta.cpu().numpy(), single, _columns(self.X))

    def svd_factors(self):
        """numpy's legacy ``multivariate_normal`` factor of every local
        covariance, A_n = sqrt(s)[:, None] * V with (U, s, V) = svd(C_n),
        as a device tensor [N, d, d] (the reference's draw,
        local_transition.py:141-145).  The production proposal kernel uses
        the Cholesky factor instead (the same distribution); this factor
        makes draws from given (u, z) equal the reference's."""
        _, s, v = np.linalg.svd(self.covs)
        return torch.as_tensor(np.sqrt(s)[..., :, None] * v,
                               device=self._Xd.device)

    def rvs_from(self, u, z):
        """Draws from the reference's random numbers: u[B] uniforms (the
        ``choice``) and z[B, d] normals (the ``multivariate_normal``), in
        the order rvs_single consumes them.  Returns (theta [B, d], idx)."""
        dev = self._Xd.device
        theta, idx, _ = K.resample_perturb_local(
            self._Xd, self._cdf, torch.as_tensor(np.asarray(u), device=dev),
            torch.as_tensor(np.asarray(z), device=dev), self.svd_factors())
        return theta, idx


class _LocalDeviceFit:
    """LocalTransition state as the generation engine consumes it:
    ``propose`` = rvs_single for a whole batch (choice by the weight CDF,
    then N(X_idx, C_idx), local_transition.py:141-145) with the prior-support
    flag, ``logpdf`` = the density pass (local_transition.py:103-110)."""

    def __init__(self, tr):
        self.X = tr._Xd
        self.w = tr._wd
        self.n = self.X.shape[0]
        self.cdf = tr._cdf
        self._covs, self._invs, self._dets = tr._covs, tr._invs, tr._dets
        self.kde_precision = tr.kde_precision

    def propose(self, lo, scale, seed, sid, offset, B):
        return K.propose_local(self.X, self.cdf, self._covs, seed, sid,
                               offset, B, lo, scale)

    def logpdf(self, theta):
        return K.local_logpdf(theta, self.X, self.w, self._invs, self._dets,
                              self.kde_precision)


def kfold_offsets(n, k):
    """The k + 1 row offsets of sklearn's unshuffled KFold: contiguous folds
    in row order, the first n % k of n // k + 1 rows, the rest of n // k."""
    q, r = divmod(int(n), int(k))
    return [f * q + min(f, r) for f in range(k + 1)]


def _first_argmax(scores):
    """Index of the first maximum (sklearn: rank 1 by ``min`` ranking)."""
    return int(np.argmax(np.asarray(scores, dtype=np.float64)))


def _take_rows(a, idx):
    if isinstance(a, pd.DataFrame):
        return a.iloc[idx]
    if isinstance(a, DeviceFrame):
        return DeviceFrame(a.tensor[torch.as_tensor(idx)], a.columns)
    if isinstance(a, torch.Tensor):
        return a[torch.as_tensor(idx)]
    return np.asarray(a)[idx]


class GridSearchCV:
    """Select transition parameters by k-fold cross-validation of the
    weighted log-likelihood ``Transition.score`` (model_selection.py:9-69,
    there a thin adapter over ``sklearn.model_selection.GridSearchCV``;
    sklearn is not needed here).

    Defaults: ``estimator = MultivariateNormalTransition()``,
    ``param_grid = {'scaling': np.linspace(0.05, 1.0, 5)}``, ``cv = 5``.
    Folds are sklearn's unshuffled ``KFold`` (:func:`kfold_offsets`), the
    mean test score is the plain mean over the folds and the first maximum
    wins.  ``scoring``, ``n_jobs``, ``iid``, ``verbose``, ``pre_dispatch``,
    ``error_score`` and ``return_train_score`` only steer sklearn's dispatch
    and are accepted and ignored.  Train scores are NOT computed and
    ``cv_results_`` carries no train keys: they would quadruple the pair
    count for a number nothing reads.

    A MultivariateNormalTransition searched over ``{'scaling': ...}`` runs
    as one device pass (kernels.kde_cv): per fold the training moments come
    from the fold slices' moments merged on the host, the training weights
    are used as they are (not renormalised), and every pair's whitened
    distance is computed once for the whole grid.  Any other estimator or
    grid, more than 32 parameters, a training set of fewer than 2 rows, a
    rank-deficient fold covariance or a host without a device take the
    plain loop (deepcopy, set_params, fit, score).  The two paths differ in
    one convention: the plain loop fits through ``Transition.fit``, which
    renormalises each fold's training weights to sum 1 (transitionmeta.py:
    17-18), so its effective sample size, hence its bandwidth, and its
    density's scale are those of the normalised weights.  For the same
    MultivariateNormalTransition the scores, and possibly the selected
    scaling, therefore depend on which path ran.

    Everything else (``rvs``, ``pdf``, ``device_fit``, ``logpdf_device``,
    ``cov``, ``X``, ``w``, ...) is forwarded to ``best_estimator_``.
    """

    def __init__(self, estimator=None, param_grid=None, scoring=None,
                 n_jobs=1, iid=True, refit=True, cv=5, verbose=0,
                 pre_dispatch='2*n_jobs', error_score='raise',
                 return_train_score=True):
        if estimator is None:
            estimator = MultivariateNormalTransition()
        if param_grid is None:
            param_grid = {'scaling': np.linspace(0.05, 1.0, 5)}
        self.estimator = estimator
        self.param_grid = param_grid
        self.refit = refit
        self.cv = cv

    def __getattr__(self, item):
        if item == "best_estimator_":
            raise AttributeError(item)
        return getattr(self.best_estimator_, item)

    def _candidates(self):
        names = sorted(self.param_grid)
        cands = [{}]
        for name in names:
            cands = [dict(c, **{name: v}) for c in cands
                     for v in self.param_grid[name]]
        return cands

    def fit(self, X, w):
        n = len(X)
        if n <= 1 or _ncols(X) == 0:
            self.estimator.fit(X, w)
            self.best_estimator_ = self.estimator
            return self
        if int(self.cv) < 2:
            raise ValueError(f"cv must be at least 2, got {self.cv}")
        k = min(int(self.cv), n)
        off = kfold_offsets(n, k)
        cands = self._candidates()
        scores = None
        if (isinstance(self.estimator, MultivariateNormalTransition)
                and list(self.param_grid) == ['scaling']
                and torch.cuda.is_available()):
            scores = self._device_scores(X, w, off)
        if scores is None:
            scores = self._host_scores(X, w, off, cands)
        mean = scores.mean(axis=0)
        best = _first_argmax(mean)
        self.best_index_ = best
        self.best_params_ = cands[best]
        self.best_score_ = float(mean[best])
        res = {"params": cands, "mean_test_score": mean,
               "std_test_score": scores.std(axis=0)}
        for name in self.param_grid:
            res["param_" + name] = np.array([c[name] for c in cands],
                                            dtype=object)
        for f in range(k):
            res[f"split{f}_test_score"] = scores[f]
        # sklearn's 'min' ranking: 1 + the number of strictly better ones
        res["rank_test_score"] = np.array(
            [1 + int(np.sum(mean > m)) for m in mean], dtype=np.int32)
        self.cv_results_ = res
        if self.refit:
            est = copy.deepcopy(self.estimator).set_params(**cands[best])
            est.fit(X, w)
            self.best_estimator_ = est
        return self

    def _host_scores(self, X, w, off, cands):
        n, k = off[-1], len(off) - 1
        scores = np.empty((k, len(cands)))
        for f in range(k):
            test = np.arange(off[f], off[f + 1])
            train = np.r_[0:off[f], off[f + 1]:n]
            w_test = _take_rows(w, test)
            if isinstance(w_test, torch.Tensor):
                w_test = w_test.cpu().numpy()
            for g, params in enumerate(cands):
                est = copy.deepcopy(self.estimator).set_params(**params)
                est.fit(_take_rows(X, train), _take_rows(w, train))
                with np.errstate(divide="ignore"):
                    scores[f, g] = est.score(_take_rows(X, test), w_test)
        return scores

    def _device_scores(self, X, w, off):
        """score[f, g] of the MVN estimator over the scaling grid through
        the cross-validation kernel, or None where it does not apply."""
        Xd, _ = as_device_matrix(X)
        wd = as_device_vector(w)
        n, d = Xd.shape
        k = len(off) - 1
        sizes = np.diff(off)
        if d > 32 or n - sizes.max() < 2:
            return None
        grid = np.asarray(list(self.param_grid['scaling']), dtype=np.float64)
        # moments of the k fold slices, merged to each fold's complement on
        # the host in fp64 (pairwise update of [sum w, sum w^2, mu, C])
        mom = torch.stack([K.weighted_moments(Xd[off[f]:off[f + 1]],
                                              wd[off[f]:off[f + 1]])
                           for f in range(k)]).cpu().numpy()
        bw_sel = self.estimator.bandwidth_selector
        mu = np.empty((k, d))
        Us = np.empty((k, d, d))
        log_pdet = np.empty(k)
        for f in range(k):
            sw = sw2 = 0.0
            m = np.zeros(d)
            C = np.zeros((d, d))
            for o in range(k):
                b = mom[o, 0]
                if o == f or not b > 0:
                    continue
                delta = mom[o, 2:2 + d] - m
                C += mom[o, 2 + d:].reshape(d, d) + np.outer(delta, delta) * (
                    sw * b / (sw + b))
                m += delta * (b / (sw + b))
                sw += b
                sw2 += mom[o, 1]
            fact = sw - sw2 / sw if sw > 0 else 0.0
            if not fact > 0:
                return None
            cov1 = C / fact * bw_sel(1.0 / sw2, d) ** 2
            U, rank, lp = K.psd_whitening(cov1)
            if rank < d or not np.all(np.isfinite(U)):
                return None
            mu[f], Us[f], log_pdet[f] = m, U, lp
        host = torch.as_tensor(np.concatenate([mu.ravel(), Us.ravel()]),
                               device=Xd.device)
        _, score = K.kde_cv(Xd, wd, off, host[:k * d].view(k, d),
                            host[k * d:].view(k, d, d), grid)
        # the Gaussian constant: c[f, g] sum_{i in f} w_i
        wsum = mom[:, 0]
        c = -0.5 * (d * K.LOG_2PI + log_pdet[:, None]
                    + d * np.log(grid)[None, :])
        with np.errstate(invalid="ignore"):
            return score.cpu().numpy() + c * wsum[:, None]
