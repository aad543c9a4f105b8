"""CPU-only checks of the exhaustive search over rotations (include/fdcm.h, "Rotations"): the library exports the three
entry points and the binding knows them, their argument checks return FDCM_EINVAL with a message before any handle is
touched, and the numpy referee (rotation_ref.py) equals the definition point by point and rotates as the oracle's
transform does."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import pyoracle
from rotation_ref import brute_peak_mask3, peak_mask3, peaks3, rot_matrix, rotate_lines, rotation_peaks_ref

EINVAL = -1
NEW_SYMBOLS = ["fdcm_exhaustive_rotations_window", "fdcm_search_exhaustive_rotations", "fdcm_score_map_rotations"]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def _rot(capi, cs, pivots=None):
    cs = np.ascontiguousarray(cs, dtype=np.float32).reshape(-1, 2)
    r = capi.Rotations(capi.fptr(cs), cs.shape[0], None)
    keep = [cs]
    if pivots is not None:
        pv = np.ascontiguousarray(pivots, dtype=np.float32)
        r.pivots = capi.fptr(pv)
        keep.append(pv)
    return r, keep


def _search(capi, fm=None, tm=None, rot=None, grid=None, k=1, rx=0, ry=0, ra=0, wrap=0, out=True):
    o, n = C.c_void_p(), C.c_int64()
    return capi.lib().fdcm_search_exhaustive_rotations(fm, tm, C.byref(rot) if rot is not None else None,
                                                       C.byref(grid) if grid is not None else None, k, rx, ry, ra, wrap, 0,
                                                       C.byref(o) if out else None, C.byref(n) if out else None)


def test_exports_and_binds_the_rotation_entry_points(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0] for s in capi.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in bound
    from openfdcm_amd.engine import DeviceFeatureMap
    import openfdcm_amd
    for f in (DeviceFeatureMap.exhaustive_rotations_window, DeviceFeatureMap.exhaustive_rotation_search,
              DeviceFeatureMap.rotation_score_map, openfdcm_amd.rotation_window, openfdcm_amd.exhaustive_rotation_search,
              openfdcm_amd.rotation_score_map):
        assert callable(f)


def test_null_pointers_are_einval(capi):
    g = capi.Grid(0, 0, 4, 4, 1, 1)
    r, keep = _rot(capi, [[1, 0]])
    assert _search(capi, rot=r, grid=g) == EINVAL and "null" in _err(capi)
    assert _search(capi, rot=r, grid=None) == EINVAL and "grid is null" in _err(capi)
    out = capi.Grid()
    assert capi.lib().fdcm_exhaustive_rotations_window(None, None, C.byref(r), 1, 1, C.byref(out)) == EINVAL
    assert "null" in _err(capi)
    assert capi.lib().fdcm_score_map_rotations(None, None, C.byref(r), C.byref(g), None) == EINVAL
    assert "null" in _err(capi)


@pytest.mark.parametrize("k", [0, 65, -1])
def test_k_out_of_range_is_einval(capi, k):
    r, keep = _rot(capi, [[1, 0]])
    assert _search(capi, rot=r, grid=capi.Grid(0, 0, 4, 4, 1, 1), k=k) == EINVAL
    assert "k must be in [1, 64]" in _err(capi)


@pytest.mark.parametrize("rx,ry,ra", [(-1, 0, 0), (0, 33, 0), (0, 0, -1), (0, 0, 33), (33, 33, 33)])
def test_radii_out_of_range_are_einval(capi, rx, ry, ra):
    r, keep = _rot(capi, [[1, 0]])
    assert _search(capi, rot=r, grid=capi.Grid(0, 0, 4, 4, 1, 1), k=4, rx=rx, ry=ry, ra=ra) == EINVAL
    assert "radii rx, ry and ra must be in [0, 32]" in _err(capi)


@pytest.mark.parametrize("wrap", [-1, 2, 7])
def test_wrap_not_boolean_is_einval(capi, wrap):
    r, keep = _rot(capi, [[1, 0]])
    assert _search(capi, rot=r, grid=capi.Grid(0, 0, 4, 4, 1, 1), wrap=wrap) == EINVAL
    assert "wrap must be 0 or 1" in _err(capi)


def test_rotation_checks_are_einval(capi):
    """Checked before the handles: null handles here, so a check that came late would report "null" instead."""
    g = capi.Grid(0, 0, 4, 4, 1, 1)
    cases = [
        (None, "rotations is null"),
        (_rot(capi, np.zeros((0, 2))), "n must be >= 1"),
        (_rot(capi, [[1, 0], [np.nan, 0]]), "c and s must be finite"),
        (_rot(capi, [[1, np.inf]]), "c and s must be finite"),
        (_rot(capi, [[-np.inf, 0], [1, 0]]), "c and s must be finite"),
    ]
    for rk, what in cases:
        r = rk[0] if rk is not None else None
        assert _search(capi, rot=r, grid=g) == EINVAL, what
        assert what in _err(capi)
        out = capi.Grid()
        assert capi.lib().fdcm_exhaustive_rotations_window(None, None, C.byref(r) if r else None, 1, 1,
                                                           C.byref(out)) == EINVAL
        assert what in _err(capi)
        assert capi.lib().fdcm_score_map_rotations(None, None, C.byref(r) if r else None, C.byref(g), None) == EINVAL
        assert what in _err(capi)
    r, keep = _rot(capi, [[1, 0]])
    out = capi.Grid()
    assert capi.lib().fdcm_exhaustive_rotations_window(None, None, C.byref(r), 0, 1, C.byref(out)) == EINVAL
    assert "strides" in _err(capi)
    r.cs = None
    assert _search(capi, rot=r, grid=g) == EINVAL and "cs is null" in _err(capi)


@pytest.mark.parametrize("grid,what", [
    ((0, 0, 4, 4, 0, 1), "stride"), ((0, 0, 0, 4, 1, 1), "nx and ny"), ((0, 0, 1 << 16, 1 << 15, 1, 1), "2^31"),
])
def test_bad_grids_are_einval(capi, grid, what):
    r, keep = _rot(capi, [[1, 0]])
    assert _search(capi, rot=r, grid=capi.Grid(*grid)) == EINVAL
    assert what in _err(capi)


def test_key_bound_is_einval(capi):
    """n_rot * nx * ny <= 2^32: N = 2^30 allows 4 rotations (the next check then finds the null handles), not 5."""
    g = capi.Grid(0, 0, 1 << 15, 1 << 15, 1, 1)
    r, keep = _rot(capi, np.tile([[1, 0]], (4, 1)))
    assert _search(capi, rot=r, grid=g) == EINVAL and "null" in _err(capi)
    r, keep = _rot(capi, np.tile([[1, 0]], (5, 1)))
    assert _search(capi, rot=r, grid=g) == EINVAL
    assert "n_rot * nx * ny must be at most 2^32" in _err(capi)


# ---------------------------------------------------------------- the referee against the definition
def _random_vol(rng, A, ny, nx, levels, nan_frac):
    m = rng.integers(0, levels, size=(A, ny, nx)).astype(np.float32) * np.float32(0.75)
    m[rng.random((A, ny, nx)) < nan_frac] = np.nan
    if ny > 3 and nx > 3:
        m[0, :2, -3:] = np.nan
    return m


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("r", [(0, 0, 0), (1, 1, 1), (2, 0, 1), (0, 3, 2), (1, 2, 4), (3, 3, 3)])
@pytest.mark.parametrize("wrap", [False, True])
def test_reference_equals_brute_force(seed, r, wrap):
    rx, ry, ra = r
    rng = np.random.default_rng(1000 * seed + 100 * rx + 10 * ry + ra + wrap)
    A = int(rng.integers(1, 8))  # includes 2 ra + 1 >= A
    ny, nx = int(rng.integers(1, 11)), int(rng.integers(1, 13))
    v = _random_vol(rng, A, ny, nx, levels=[2, 3, 6, 40, 1][seed], nan_frac=[0, 0.1, 0.3, 0.05, 0.5][seed])
    assert np.array_equal(peak_mask3(v, rx, ry, ra, wrap), brute_peak_mask3(v, rx, ry, ra, wrap))


def test_reference_ties_and_wrap():
    """All zero: the lowest angle, then the lowest grid index wins; with wrap, angle 0's window holds angle A - 1."""
    v = np.zeros((6, 4, 5), dtype=np.float32)
    for wrap in (False, True):
        assert np.argwhere(peak_mask3(v, 1, 1, 1, wrap)).tolist() == [[0, 0, 0]]
        assert np.argwhere(peak_mask3(v, 32, 32, 2, wrap)).tolist() == [[0, 0, 0]]
        # ra only: every grid point's lowest angle
        assert np.array_equal(peak_mask3(v, 0, 0, 1, wrap), np.arange(6)[:, None, None] == np.zeros((1, 4, 5)))
    # a single grid point: with ra = 1 every angle but 0 has a lower neighbour; with ra = 0 all are peaks
    assert np.argwhere(peak_mask3(v[:, :1, :1], 0, 0, 1, False)).tolist() == [[0, 0, 0]]
    assert np.argwhere(peak_mask3(v[:, :1, :1], 0, 0, 0, False)).tolist() == [[a, 0, 0] for a in range(6)]
    w = np.ones((6, 4, 5), dtype=np.float32)
    w[5, 2, 2] = 0.5
    w[0, 2, 2] = 0.5  # a tie across the wrap: angle 0 wins, angle 5 is no peak with wrap
    assert peak_mask3(w, 0, 0, 1, True)[0, 2, 2] and not peak_mask3(w, 0, 0, 1, True)[5, 2, 2]
    assert peak_mask3(w, 0, 0, 1, False)[5, 2, 2]
    # r = 0: every admissible point, in (score, a, g) order
    a, g, s = peaks3(np.array([[[2, 1]], [[1, np.nan]]], dtype=np.float32), 64, 0, 0, 0, False)
    assert list(a) == [0, 1, 0] and list(g) == [1, 0, 0] and list(s) == [1, 1, 2]


@pytest.mark.parametrize("cs", [(1, 0), (0, 1), (-1, 0), (np.cos(0.3), np.sin(0.3)), (1.5 * np.cos(2), 1.5 * np.sin(2))])
@pytest.mark.parametrize("pivot", [(0, 0), (3.25, -7.5), (101.7, 55.1)])
def test_rotation_is_the_oracle_transform_of_rotate(cs, pivot):
    """M_a as math.h's rotate(lines, R, rot_point) builds it: transl = rot_point - R rot_point; then pyoracle.transform."""
    rng = np.random.default_rng(5)
    lines = (rng.random((4, 17)) * 200 - 50).astype(np.float32)
    c, s = np.float32(cs[0]), np.float32(cs[1])
    R = np.array([[c, -s], [s, c]], dtype=np.float32)
    p = np.array(pivot, dtype=np.float32)
    Rp = np.array([R[0, 0] * p[0] + R[0, 1] * p[1], R[1, 0] * p[0] + R[1, 1] * p[1]], dtype=np.float32)
    M = np.zeros((2, 3), dtype=np.float32)
    M[:, :2] = R
    M[:, 2] = p - Rp
    assert np.array_equal(rot_matrix(c, s, *p), M)
    want = pyoracle.transform(lines, M)
    got = rotate_lines(lines, c, s, *p)
    assert want.dtype == np.float32 and got.tobytes() == want.tobytes()


def test_reference_records():
    v = np.full((2, 3, 2, 4), np.nan, dtype=np.float32)
    v[0, 1, 1, 2] = 0.5
    v[0, 2, 0, 0] = 0.25
    cs = np.array([[1, 0], [0, 1], [-1, 0]], dtype=np.float32)
    recs = rotation_peaks_ref(v, cs, np.array([[2, 3], [0, 0]], dtype=np.float32), 4, 2, 1, 1, True,
                              grid=(-4, 10, 4, 2, 3, 2), base=5)
    assert list(recs["tmpl_idx"]) == [5] and list(recs["score"]) == [0.25]
    M = rot_matrix(-1, 0, 2, 3)
    assert np.array_equal(recs["transform"][0], [M[0, 0], M[0, 1], M[0, 2] - 4, M[1, 0], M[1, 1], M[1, 2] + 10])
    recs = rotation_peaks_ref(v, cs, None, 4, 0, 0, 0, False, grid=(-4, 10, 4, 2, 3, 2))
    assert list(recs["score"]) == [0.25, 0.5] and recs["transform"][1][2] == -4 + 2 * 3
