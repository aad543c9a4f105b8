"""CPU-only checks of the exhaustive search's peaks (include/fdcm.h, "Peaks"): the library exports
fdcm_search_exhaustive_peaks and the binding knows it, its argument checks return FDCM_EINVAL with a message before any
handle is touched, and the numpy referee (peaks_ref.py) equals the definition point by point."""
import ctypes as C
import os

import numpy as np
import pytest

from peaks_ref import brute_peak_mask, peak_mask, peaks, peaks_ref

EINVAL = -1


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def _call(capi, fm=None, tm=None, grid=None, k=1, rx=0, ry=0, out=True):
    o, n = C.c_void_p(), C.c_int64()
    g = C.byref(grid) if grid is not None else None
    return capi.lib().fdcm_search_exhaustive_peaks(fm, tm, g, k, rx, ry, 0, C.byref(o) if out else None,
                                                   C.byref(n) if out else None)


def test_exports_and_binds_the_peaks_entry_point(capi):
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "fdcm_search_exhaustive_peaks")
    assert "fdcm_search_exhaustive_peaks" in {s[0] for s in capi.SYMBOLS}
    from openfdcm_amd.engine import DeviceFeatureMap
    import openfdcm_amd
    assert callable(DeviceFeatureMap.exhaustive_peaks) and callable(openfdcm_amd.exhaustive_peaks)


def test_null_pointers_are_einval(capi):
    g = capi.Grid(0, 0, 4, 4, 1, 1)
    assert _call(capi, grid=g) == EINVAL
    assert "null" in _err(capi)
    assert _call(capi, grid=None) == EINVAL
    assert "grid is null" in _err(capi)


@pytest.mark.parametrize("grid,what", [
    ((0, 0, 4, 4, 0, 1), "stride"), ((0, 0, 4, 4, 1, -2), "stride"),
    ((0, 0, 0, 4, 1, 1), "nx and ny"), ((0, 0, 4, -1, 1, 1), "nx and ny"),
    ((0, 0, 1 << 16, 1 << 15, 1, 1), "2^31"),
])
def test_bad_grids_are_einval(capi, grid, what):
    assert _call(capi, grid=capi.Grid(*grid)) == EINVAL
    assert what in _err(capi)


@pytest.mark.parametrize("k", [0, 65, -1])
def test_k_out_of_range_is_einval(capi, k):
    assert _call(capi, grid=capi.Grid(0, 0, 4, 4, 1, 1), k=k) == EINVAL
    assert "k must be in [1, 64]" in _err(capi)


@pytest.mark.parametrize("rx,ry", [(-1, 0), (0, -1), (33, 0), (0, 33), (-1, 33)])
def test_radii_out_of_range_are_einval(capi, rx, ry):
    assert _call(capi, grid=capi.Grid(0, 0, 4, 4, 1, 1), k=4, rx=rx, ry=ry) == EINVAL
    assert "radii rx and ry must be in [0, 32]" in _err(capi)


# ---------------------------------------------------------------- the referee against the definition
def _random_map(rng, ny, nx, levels, nan_frac):
    """Scores from a few levels (ties and plateaus), NaN holes, and a NaN block at an edge."""
    m = rng.integers(0, levels, size=(ny, nx)).astype(np.float32) * np.float32(0.75)
    m[rng.random((ny, nx)) < nan_frac] = np.nan
    if ny > 3 and nx > 3:
        m[:2, -3:] = np.nan
    return m


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("rx,ry", [(0, 0), (1, 1), (3, 1), (0, 5), (2, 7), (8, 8)])
def test_reference_equals_brute_force(seed, rx, ry):
    rng = np.random.default_rng(100 * seed + 7 * rx + ry)
    ny, nx = int(rng.integers(1, 23)), int(rng.integers(1, 29))
    m = _random_map(rng, ny, nx, levels=[2, 3, 6, 50, 1000, 4][seed], nan_frac=[0, 0.1, 0.3, 0.05, 0.2, 0.6][seed])
    assert np.array_equal(peak_mask(m, rx, ry), brute_peak_mask(m, rx, ry))


def test_reference_plateau_and_edges():
    """Equal scores: a point is a peak when no lower grid index is admissible within the radius.  A full plateau keeps
    only its first point; admissible points on a lattice of steps (rx + 1, ry + 1) are all peaks, on steps (rx, ry) only
    the first; all NaN keeps none."""
    m = np.zeros((10, 13), dtype=np.float32)
    for rx, ry in [(1, 2), (32, 32), (1, 1)]:
        one = peak_mask(m, rx, ry)
        assert one.sum() == 1 and one[0, 0]
    assert np.argwhere(peak_mask(m, 0, 1)).tolist() == [[0, i] for i in range(13)]  # ry only: the first row
    assert np.argwhere(peak_mask(m, 4, 0)).tolist() == [[j, 0] for j in range(10)]  # rx only: the first column
    lattice = np.full_like(m, np.nan)
    lattice[::3, ::2] = 0
    assert np.array_equal(peak_mask(lattice, 1, 2), lattice == 0)
    assert np.array_equal(brute_peak_mask(lattice, 1, 2), lattice == 0)
    assert np.argwhere(peak_mask(lattice, 2, 3)).tolist() == [[0, 0]]
    assert not peak_mask(np.full((4, 4), np.nan, dtype=np.float32), 1, 1).any()
    # r = 0: every admissible point, in (score, g) order
    m = np.array([[2, np.nan, 1], [1, 0, 2]], dtype=np.float32)
    g, s = peaks(m, 64, 0, 0)
    assert list(g) == [4, 2, 3, 0, 5] and list(s) == [0, 1, 1, 2, 2]


def test_reference_records():
    m = np.array([[[3, 1, 3, 3, 0.5], [3, 3, 3, 3, 3]], [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]], dtype=np.float32)
    recs = peaks_ref(m, 8, 1, 1, grid=(-4, 10, 5, 2, 3, 2), base=5)
    assert list(recs["tmpl_idx"]) == [5, 5, 6]
    assert list(recs["score"]) == [0.5, 1, 0]
    assert list(recs["transform"][:, 2]) == [-4 + 4 * 3, -4 + 3, -4]
    assert list(recs["transform"][:, 5]) == [10, 10, 10]
    assert list(recs["transform"][:, 0]) == [1, 1, 1] and list(recs["transform"][:, 4]) == [1, 1, 1]
    assert len(peaks_ref(m, 8, 1, 1, grid=(0, 0, 5, 2, 1, 1), skip={0, 1})) == 0
