"""GridSearchCV's host rules (no GPU): sklearn's unshuffled KFold offsets and
the first-maximum tie rule."""
import numpy as np
import pytest

from pyabc_amd.transition import _first_argmax, kfold_offsets


@pytest.mark.parametrize("n,k", [(7, 3), (10, 5), (9, 9), (131, 5)])
def test_kfold_offsets(n, k):
    off = kfold_offsets(n, k)
    sizes = np.diff(off)
    assert len(off) == k + 1 and off[0] == 0 and off[-1] == n
    assert list(sizes) == [n // k + 1] * (n % k) + [n // k] * (k - n % k)


def test_first_maximum_wins_a_tie():
    table = np.array([[-3.0, -1.0, -1.0, -2.0],
                      [-1.0, -2.0, -2.0, -1.0]])      # means -2, -1.5, -1.5, -1.5
    assert _first_argmax(table.mean(0)) == 1
    assert _first_argmax([-np.inf, -np.inf]) == 0
