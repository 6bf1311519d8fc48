"""MassActionODEModel on the host: bad network descriptions are refused
before anything reaches the device, and the compiled table is the network."""
import numpy as np
import pytest
import torch

T10 = np.linspace(1, 10, 10)
AB = ({"A": 1}, {"B": 1}, 1.0)

BAD = {
    "unknown species": (["A", "B"], [({"A": 1}, {"C": 1}, 1.0)], [1, 0], T10, None),
    "unknown observed": (["A", "B"], [AB], [1, 0], T10, ["C"]),
    "order 3": (["A", "B"], [({"A": 2, "B": 1}, {}, 1.0)], [1, 0], T10, None),
    "9 species": ([f"X{i}" for i in range(9)], [({"X0": 1}, {}, 1.0)],
                  [0.0] * 9, T10, None),
    "17 reactions": (["A", "B"], [AB] * 17, [1, 0], T10, None),
    "S = 258": (["A", "B"], [AB], [1, 0], np.arange(1, 130), None),
    "times not increasing": (["A", "B"], [AB], [1, 0], [1.0, 2.0, 2.0], None),
}


@pytest.mark.parametrize("case", list(BAD))
def test_bad_description_raises(case):
    import pyabc_amd as pa
    species, reactions, x_init, t_obs, observed = BAD[case]
    with pytest.raises(ValueError):
        pa.MassActionODEModel(species, reactions, x_init, t_obs, observed=observed)


def test_theta_column_checked_at_simulate_time():
    import pyabc_amd as pa
    m = pa.MassActionODEModel(["A", "B"], [({"A": 1}, {"B": 1}, ("theta", 1))],
                              [1, 0], T10)
    with pytest.raises(ValueError):
        m.simulate(torch.zeros((4, 1), dtype=torch.float64), 0, 0, 0)
    with pytest.raises(ValueError):
        m.simulate_host(np.zeros((4, 1)))


def test_compiled_table_of_dimerisation():
    """2A -> B (10 ** theta_0), B -> 2A (theta_1), B -> 0 (0.3)"""
    import pyabc_amd as pa
    m = pa.MassActionODEModel(
        ["A", "B"], [({"A": 2}, {"B": 1}, ("log10theta", 0)),
                     ({"B": 1}, {"A": 2}, ("theta", 1)), ({"B": 1}, {}, 0.3)],
        [1.0, ("theta", 2)], T10, observed=["B"])
    assert m.reactant_slots == [(0, 0), (1, -1), (1, -1)]
    assert m.net == [[(0, -2), (1, 1)], [(0, 2), (1, -1)], [(1, -1)]]
    t = m.table
    assert (t.n_species, t.n_reactions, t.n_times, t.n_observed) == (2, 3, 10, 1)
    assert [list(r) for r in t.reactant[:3]] == [[0, 0], [1, -1], [1, -1]]
    assert list(t.pair_start[:4]) == [0, 2, 4, 5]
    assert [(p & 0xff, p >> 8) for p in t.pair[:5]] == \
        [(0, -2), (1, 1), (0, 2), (1, -1), (1, -1)]
    assert list(t.rate_kind[:3]) == [2, 1, 0] and list(t.rate_col[:2]) == [0, 1]
    assert t.rate_const[2] == 0.3
    assert list(t.x_init_col[:2]) == [-1, 2] and t.x_init[0] == 1.0
    assert t.observed[0] == 1 and list(t.t_obs[:10]) == list(T10)
    assert m.keys == tuple(f"B_{j:03d}" for j in range(10))
