"""MassActionSSAModel without a GPU: bad descriptions and bad C-call
arguments are refused before anything reaches the device, and no
instantiation of the kernels spills a register or uses scratch."""
import ctypes
import os

import numpy as np
import pytest

from tools import spill_report as sr

T10 = np.linspace(1, 10, 10)
DEATH = ({"A": 1}, {}, 1.0)

BAD = {
    "fractional count": dict(x_init=[2.5]),
    "negative count": dict(x_init=[-1]),
    "order 3": dict(reactions=[({"A": 3}, {}, 1.0)]),
    "max_events 0": dict(max_events=0),
    "max_events > 2^24": dict(max_events=(1 << 24) + 1),
}


@pytest.mark.parametrize("case", list(BAD))
def test_bad_description_raises(case):
    import pyabc_amd as pa
    kw = dict(species=["A"], reactions=[DEATH], x_init=[5], t_obs=T10)
    kw.update(BAD[case])
    with pytest.raises(ValueError):
        pa.MassActionSSAModel(**kw)


# (B, d, max_events, offset, ld, fractional constant count) -> message part
BAD_CALL = [
    ((4, 1, 0, 0, 4, False), b"max_events"),
    ((4, 1, (1 << 24) + 1, 0, 4, False), b"max_events"),
    ((4, 1, 10, (1 << 40) - 3, 4, False), b"offset + B"),
    ((4, 1, 10, 0, 3, False), b"bad sizes"),
    ((4, 33, 10, 0, 4, False), b"bad sizes"),
    ((4, 1, 10, 0, 4, True), b"must be an integer"),
]


@pytest.mark.parametrize("args,msg", BAD_CALL)
def test_c_call_argument_errors(args, msg):
    import pyabc_amd as pa
    from pyabc_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built")
    lib = _native.lib()
    B, d, max_events, offset, ld, fractional = args
    table = pa.MassActionSSAModel(["A"], [DEATH], [5], T10).table
    if fractional:
        table.x_init[0] = 2.5
    rc = lib.abc_sim_mass_action_ssa_f64(ctypes.byref(table), None, B, d,
                                         max_events, 1, 2, offset, None, ld,
                                         None, None)
    assert rc == -1 and msg in lib.abc_last_error()


@pytest.mark.skipif(not os.path.exists(sr.DEFAULT_LIB) or sr.readelf() is None,
                    reason="built library or llvm-readelf missing")
def test_no_spills_no_scratch():
    res = sr.kernel_resources()
    dm = sr.demangle(list(res))
    got = {dm[k]: v for k, v in res.items() if "abc::ssa_" in dm[k]}
    assert len(got) == 17      # two forms at n = 1 .. 8 and the counter reset
    for name, r in got.items():
        assert not any(r.get(f, 0) for f in (
            "sgpr_spill_count", "vgpr_spill_count",
            "private_segment_fixed_size")), (name, r)
