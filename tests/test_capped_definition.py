"""CPU-only checks of the capped score's definition as the referee states it (capped_ref.py): the vectorised Eigen-order
sum against the oracle's eigen_sum for every length from 0 to 40, and the clamp on hand cases."""
import numpy as np
import pytest

from capped_ref import capped_volumes, clamp, eigen_sum0, one_line_set
from oracle.pyoracle import eigen_sum

INF, NAN = np.float32(np.inf), np.float32(np.nan)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("n", range(41))
def test_vectorised_sum_is_eigens(n):
    """Random magnitudes over many binades, so the order of the additions shows in the bits."""
    rng = np.random.default_rng(n)
    v = (rng.uniform(0, 1, size=(n, 7, 5)) * 10.0 ** rng.integers(-3, 6, size=(n, 7, 5))).astype(np.float32)
    got = eigen_sum0(v)
    assert got.shape == (7, 5) and got.dtype == np.float32
    for j in range(7):
        for i in range(5):
            assert _bits(got[j, i]) == _bits(eigen_sum(v[:, j, i])), (n, j, i)


def test_sum_carries_nan_and_inf():
    v = np.ones((9, 3), dtype=np.float32)
    v[5, 0], v[8, 1] = NAN, INF
    got = eigen_sum0(v)
    assert np.isnan(got[0]) and np.isinf(got[1]) and got[2] == 9


def test_clamp_hand_cases():
    assert np.isnan(clamp(NAN, 3.0)) and np.isnan(clamp(NAN, INF)) and np.isnan(clamp(NAN, 0.0))  # NaN stays
    assert clamp(INF, 3.0) == 3 and clamp(INF, 0.0) == 0                                        # inf under a finite cap
    assert np.isinf(clamp(INF, INF))
    assert clamp(7.5, 0.0) == 0 and _bits(clamp(0.0, 0.0)) == 0                                  # cap 0 switches a line off
    assert clamp(2.0, 3.0) == 2 and clamp(3.0, 3.0) == 3 and clamp(3.5, 3.0) == 3
    rng = np.random.default_rng(1)
    v = rng.uniform(0, 1e6, size=100).astype(np.float32)
    v[::7] = INF
    v[::11] = NAN
    assert np.array_equal(_bits(clamp(v, INF)), _bits(v))                                       # +inf is the identity
    assert clamp(v, 5.0).dtype == np.float32


def test_capped_volumes_on_a_hand_case():
    """Two templates on a 1 x 3 map: sums of clamped costs where the template's own map is not NaN, NaN elsewhere; a
    template without lines is +0 where admissible."""
    tm = [np.zeros((4, 2), dtype=np.float32), np.zeros((4, 0), dtype=np.float32)]
    lines, offsets = one_line_set(tm)
    assert len(lines) == 2 and offsets.tolist() == [0, 2, 2] and lines[0].shape == (4, 1)
    cost = np.float32([[[1, 9, 4]], [[INF, 2, NAN]]])
    uncapped = np.float32([[[INF, 11, NAN]], [[0, 0, NAN]]])
    got = capped_volumes(cost, offsets, [np.float32([3, 5]), np.zeros(0, np.float32)], uncapped)
    assert got[0, 0, :2].tolist() == [6, 5] and np.isnan(got[0, 0, 2])
    assert got[1, 0, :2].tolist() == [0, 0] and np.isnan(got[1, 0, 2])
    same = capped_volumes(cost, offsets, [np.float32([INF, INF]), np.zeros(0, np.float32)], uncapped)
    assert np.array_equal(_bits(same), _bits(uncapped))
