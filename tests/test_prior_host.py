"""Distribution.device_table: which priors the device table can hold, and
how loc / scale are read (no GPU)."""
import numpy as np
import pytest
import scipy.stats as st

import pyabc_amd as pa
from pyabc_amd._native import PriorTable as P

SHAPES = {"uniform": (), "norm": (), "lognorm": (0.7,), "expon": (),
          "laplace": (), "loguniform": (0.01, 100.0), "reciprocal": (1.0, 2.0),
          "truncnorm": (-1.5, 4.0), "gamma": (2.5,), "beta": (0.5, 2.0)}


@pytest.mark.parametrize("fam", list(SHAPES))
def test_table_for_each_family_positional_and_keyword(fam):
    sh = SHAPES[fam]
    tabs = [pa.Distribution(x=rv).device_table() for rv in (
        pa.RV(fam, *sh, 1.5, 2.0), pa.RV(fam, *sh, loc=1.5, scale=2.0),
        pa.RV(fam, *sh, 1.5, scale=2.0))]
    assert all(t is not None and t[0] == ["x"] for t in tabs)
    assert len({t[1].key() for t in tabs}) == 1
    t = tabs[0][1]
    assert (t.loc[0], t.scale[0]) == (1.5, 2.0)
    assert t.family[0] == pa.random_variables.DEVICE_FAMILIES[fam]
    lo, hi = getattr(st, fam).support(*sh)
    assert (t.zlo[0], t.zhi[0]) == (lo, hi)
    # the constant is the log density where every z term vanishes or is known
    z = {"uniform": 0.5, "norm": 0.0, "laplace": 0.0, "expon": 0.0}.get(fam)
    if z is not None:
        assert t.c[0] == pytest.approx(
            pa.RV(fam, *sh, 1.5, 2.0).logpdf(1.5 + 2.0 * z), rel=1e-15)


def test_sorted_names_and_closed_ends():
    names, t = pa.Distribution(b=pa.RV("gamma", 3.0), a=pa.RV("gamma", 0.5),
                               c=pa.RV("uniform", 0, 1)).device_table()
    assert names == ["a", "b", "c"]
    assert [bool(t.mask[i] & P.LO_CLOSED) for i in range(3)] == [True, False,
                                                                 True]
    assert t.mask[2] & P.HI_CLOSED and not t.mask[0] & P.HI_CLOSED


@pytest.mark.parametrize("rv", [
    pa.LowerBoundDecorator(pa.RV("norm", 0, 1), -1.0), pa.RV("poisson", 3.0),
    pa.RV("cauchy"), pa.RV("norm", 0, np.inf), pa.RV("uniform", 0, 0)],
    ids=["decorated", "discrete", "unknown", "inf-scale", "zero-scale"])
def test_no_table(rv):
    assert pa.Distribution(x=pa.RV("norm", 0, 1), y=rv).device_table() is None


def test_uniform_box_unchanged():
    prior = pa.Distribution(b=pa.RV("uniform", -1, 3), a=pa.RV("uniform", 2, 5))
    names, lo, sc = prior.uniform_box()
    assert names == ["a", "b"] and list(lo) == [2, -1] and list(sc) == [5, 3]
    assert pa.Distribution(a=pa.RV("norm", 0, 1)).uniform_box() is None
    assert prior.device_table() is not None


def test_batch_spec_takes_table_priors_when_asked():
    from pyabc_amd.sampler.gpu import BatchSpec

    def reason(rv, **kw):
        return BatchSpec(
            1, "smc", [pa.GaussianMeanModel()], priors=[pa.Distribution(a=rv)],
            transitions=[pa.MultivariateNormalTransition()],
            distance=pa.PNormDistance(), eps=pa.MedianEpsilon(),
            acceptor=pa.UniformAcceptor(), x_0={"data": 1.0},
            nr_samples_per_parameter=1,
            summary_statistics=pa.smc.identity).unsupported_reason(**kw)
    assert reason(pa.RV("norm", 0, 1), prior_table=True) is None
    assert "uniform" in reason(pa.RV("norm", 0, 1))
    assert "device table" in reason(pa.RV("cauchy"), prior_table=True)
