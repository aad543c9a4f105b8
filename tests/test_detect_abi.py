"""CPU-only checks of the best map and the detections (include/fdcm.h, "Best map and detections"): the library exports
fdcm_best_map and fdcm_search_exhaustive_detect and the binding knows them, their argument checks return FDCM_EINVAL with
a message before any handle is touched, and the numpy referee (detect_ref.py) equals its point-by-point form."""
import ctypes as C
import os

import numpy as np
import pytest

from detect_ref import best_ref, brute_best, brute_detect, detect_ref, normalised, pair_keys
from peaks_ref import NO_KEY

EINVAL = -1
NEW_SYMBOLS = ["fdcm_best_map", "fdcm_search_exhaustive_detect"]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def _rot(capi, cs):
    cs = np.ascontiguousarray(cs, dtype=np.float32).reshape(-1, 2)
    return capi.Rotations(capi.fptr(cs), cs.shape[0], None), cs


def _detect(capi, rot=None, grid=None, k=1, rx=0, ry=0, penalty=-1, tau=1.0, out=True):
    o, n = C.c_void_p(), C.c_int64()
    return capi.lib().fdcm_search_exhaustive_detect(None, None, C.byref(rot) if rot is not None else None,
                                                    C.byref(grid) if grid is not None else None, k, rx, ry, penalty, tau, 0,
                                                    C.byref(o) if out else None, C.byref(n) if out else None)


def _best(capi, rot=None, grid=None, penalty=-1, tau=1.0, outs=(True, True)):
    s, p = np.zeros(16, dtype=np.float32), np.zeros(16, dtype=np.int32)
    return capi.lib().fdcm_best_map(None, None, C.byref(rot) if rot is not None else None,
                                    C.byref(grid) if grid is not None else None, penalty, tau, capi.fptr(s) if outs[0] else None,
                                    p.ctypes.data_as(C.POINTER(C.c_int32)) if outs[1] else None)


def test_exports_and_binds_the_entry_points(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0] for s in capi.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in bound
    from openfdcm_amd.engine import DeviceFeatureMap
    import openfdcm_amd
    for f in (DeviceFeatureMap.best_map, DeviceFeatureMap.exhaustive_detect, openfdcm_amd.best_score_map,
              openfdcm_amd.exhaustive_detect):
        assert callable(f)
    with open(os.path.join(os.path.dirname(capi.LIB_PATH), "..", "include", "fdcm.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert "int " + name + "(" in header


def test_null_pointers_are_einval(capi):
    g = capi.Grid(0, 0, 4, 4, 1, 1)
    assert _detect(capi, grid=g) == EINVAL and "null featuremap/templates" in _err(capi)  # rot may be null, the handles not
    assert _best(capi, grid=g) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _detect(capi, grid=None) == EINVAL and "grid is null" in _err(capi)
    assert _best(capi, grid=None) == EINVAL and "grid is null" in _err(capi)
    assert _detect(capi, grid=g, out=False) == EINVAL and "null output" in _err(capi)
    assert _best(capi, grid=g, outs=(False, False)) == EINVAL and "both null" in _err(capi)
    for outs in [(True, False), (False, True)]:  # either may be null: the call goes on to the handles
        assert _best(capi, grid=g, outs=outs) == EINVAL and "null featuremap/templates" in _err(capi)


@pytest.mark.parametrize("grid,what", [
    ((0, 0, 4, 4, 0, 1), "stride"), ((0, 0, 4, 4, 1, -2), "stride"),
    ((0, 0, 0, 4, 1, 1), "nx and ny"), ((0, 0, 4, -1, 1, 1), "nx and ny"),
    ((0, 0, 1 << 16, 1 << 15, 1, 1), "2^26"), ((0, 0, (1 << 13) + 1, 1 << 13, 1, 1), "2^26"), ((0, 0, (1 << 26) + 1, 1, 1, 1), "2^26"),
])
def test_bad_grids_are_einval(capi, grid, what):
    assert _detect(capi, grid=capi.Grid(*grid)) == EINVAL and what in _err(capi)
    assert _best(capi, grid=capi.Grid(*grid)) == EINVAL and what in _err(capi)


def test_grid_of_2_26_points_passes_the_grid_checks(capi):
    """The bound is inclusive: at 2^26 points the call goes on to the handles."""
    for g in [(0, 0, 1 << 13, 1 << 13, 1, 1), (-5, 7, 1 << 26, 1, 1, 1)]:
        assert _detect(capi, grid=capi.Grid(*g)) == EINVAL and "null featuremap/templates" in _err(capi)
        assert _best(capi, grid=capi.Grid(*g)) == EINVAL and "null featuremap/templates" in _err(capi)


@pytest.mark.parametrize("k", [0, 65, -1])
def test_k_out_of_range_is_einval(capi, k):
    assert _detect(capi, grid=capi.Grid(0, 0, 4, 4, 1, 1), k=k) == EINVAL
    assert "k must be in [1, 64]" in _err(capi)


@pytest.mark.parametrize("rx,ry", [(-1, 0), (0, -1), (33, 0), (0, 33), (-1, 33)])
def test_radii_out_of_range_are_einval(capi, rx, ry):
    assert _detect(capi, grid=capi.Grid(0, 0, 4, 4, 1, 1), k=4, rx=rx, ry=ry) == EINVAL
    assert "radii rx and ry must be in [0, 32]" in _err(capi)


@pytest.mark.parametrize("penalty", [-2, 2, 7])
def test_unknown_penalty_is_einval(capi, penalty):
    g = capi.Grid(0, 0, 4, 4, 1, 1)
    assert _detect(capi, grid=g, penalty=penalty) == EINVAL and "unknown penalty" in _err(capi)
    assert _best(capi, grid=g, penalty=penalty) == EINVAL and "unknown penalty" in _err(capi)


@pytest.mark.parametrize("tau", [np.nan, np.inf, -np.inf])
def test_tau_not_finite_is_einval(capi, tau):
    g = capi.Grid(0, 0, 4, 4, 1, 1)
    for penalty in (-1, capi.DEFAULT_PENALTY, capi.EXPONENTIAL_PENALTY):
        assert _detect(capi, grid=g, penalty=penalty, tau=tau) == EINVAL and "tau must be finite" in _err(capi)
        assert _best(capi, grid=g, penalty=penalty, tau=tau) == EINVAL and "tau must be finite" in _err(capi)


def test_known_penalties_pass_the_penalty_checks(capi):
    g = capi.Grid(0, 0, 4, 4, 1, 1)
    for penalty in (-1, capi.DEFAULT_PENALTY, capi.EXPONENTIAL_PENALTY):
        assert _detect(capi, grid=g, penalty=penalty, tau=1.5) == EINVAL and "null featuremap/templates" in _err(capi)


def test_rotation_checks_are_einval(capi):
    """What the rotation call rejects about a table, when there is one; checked before the handles (null here)."""
    g = capi.Grid(0, 0, 4, 4, 1, 1)
    for cs, what in [(np.zeros((0, 2)), "n must be >= 1"), ([[1, 0], [np.nan, 0]], "c and s must be finite"),
                     ([[1, np.inf]], "c and s must be finite")]:
        r, keep = _rot(capi, cs)
        assert _detect(capi, rot=r, grid=g) == EINVAL and what in _err(capi)
        assert _best(capi, rot=r, grid=g) == EINVAL and what in _err(capi)
    r = capi.Rotations(None, 3, None)
    assert _detect(capi, rot=r, grid=g) == EINVAL and "cs is null" in _err(capi)
    assert _best(capi, rot=r, grid=g) == EINVAL and "cs is null" in _err(capi)


# ---------------------------------------------------------------- the referee against its point-by-point form
def _random_volume(rng, T, A, ny, nx, levels, nan_frac):
    """Scores from a few levels (ties between templates and angles), NaN holes, an edge block where every pair is NaN
    (points without candidates) and one template that is NaN everywhere."""
    v = rng.integers(0, levels, size=(T, A, ny, nx)).astype(np.float32) * np.float32(0.75)
    v[rng.random(v.shape) < nan_frac] = np.nan
    if ny > 3 and nx > 3:
        v[:, :, :2, -3:] = np.nan
    if T > 2:
        v[2] = np.nan
    return v


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("rx,ry", [(0, 0), (1, 1), (3, 1), (0, 5), (2, 7), (8, 8)])
def test_reference_equals_brute_force(capi, seed, rx, ry):
    rng = np.random.default_rng(100 * seed + 7 * rx + ry)
    T, A = int(rng.integers(1, 6)), int(rng.integers(1, 4))
    ny, nx = int(rng.integers(1, 19)), int(rng.integers(1, 23))
    v = _random_volume(rng, T, A, ny, nx, levels=[2, 3, 6, 50, 1000, 4][seed], nan_frac=[0, 0.1, 0.3, 0.05, 0.2, 0.6][seed])
    lengths = rng.choice(np.float32([0.0, 1.0, 2.0, 3.5, 40.25]), size=T)
    penalty, tau = [(None, 1.0), (capi.DEFAULT_PENALTY, 1.0), (capi.EXPONENTIAL_PENALTY, 1.5)][seed % 3]
    skip = {0} if seed in (1, 4) and T > 1 else set()
    q = normalised(v, lengths, penalty, tau)
    scores, pairs = best_ref(q, skip)
    bs, bp = brute_best(q, skip)
    assert np.array_equal(pairs, bp)
    assert np.array_equal(scores.view(np.uint32), bs.view(np.uint32))
    assert np.array_equal(pairs == -1, np.isnan(scores))
    grid = (-3, 5, nx, ny, 2, 3)
    cs = None if A == 1 else np.float32([[1, 0], [0, 1], [-1, 0]])[:A]
    for k in (1, 5, 64):
        recs = detect_ref(q, k, rx, ry, grid, cs=cs, skip=skip)
        g, bits, u = brute_detect(q, k, rx, ry, skip)
        assert len(recs) == len(g)
        assert np.array_equal(recs["score"].view(np.uint32), bits)
        assert np.array_equal(recs["tmpl_idx"], u // A)
        assert np.array_equal(recs["transform"][:, 2], np.float32(-3 + (g % nx) * 2))  # (no pivot: m = 0)
        assert np.array_equal(recs["transform"][:, 5], np.float32(5 + (g // nx) * 3))
        if cs is not None:
            assert np.array_equal(recs["transform"][:, 0], cs[u % A, 0]) and np.array_equal(recs["transform"][:, 3], cs[u % A, 1])


def test_reference_normalised_scores(capi):
    """q is fdcm_penalize's value: score / max(len, 1e-6) and score / pow(max(len, 1e-6), tau) in float32; None leaves the
    scores; NaN and inf pass through."""
    v = np.float32([[[[3.0, 0.0, np.nan, np.inf]]], [[[3.0, 1.0, 2.0, 0.5]]]])
    lengths = np.float32([2.0, 0.0])
    assert np.array_equal(normalised(v, lengths, None), v, equal_nan=True)
    q = normalised(v, lengths, capi.DEFAULT_PENALTY)
    assert np.array_equal(q[0], v[0] / np.float32(2.0), equal_nan=True)
    assert np.array_equal(q[1], v[1] / np.float32(1e-6))
    q = normalised(v, lengths, capi.EXPONENTIAL_PENALTY, 1.5)
    assert np.allclose(q[0, 0, 0, :2], v[0, 0, 0, :2] / np.float32(2.0) ** np.float32(1.5), rtol=1e-6)
    assert np.isnan(q[0, 0, 0, 2]) and np.isinf(q[0, 0, 0, 3])


def test_reference_ties_skips_and_empty_points():
    """Equal q: the lowest template, then the lowest angle.  A skipped template never wins; an infinite q is a candidate
    that loses to every finite one; a point where all is NaN has no candidate."""
    q = np.zeros((3, 2, 2, 3), dtype=np.float32)
    scores, pairs = best_ref(q)
    assert np.all(pairs == 0) and np.all(scores == 0)
    scores, pairs = best_ref(q, skip={0})
    assert np.all(pairs == 2)
    q[1, 0] = np.nan
    scores, pairs = best_ref(q, skip={0})
    assert np.all(pairs == 3)
    q[:] = np.nan
    q[2, 1, 0, 0] = np.inf
    q[1, 1, 0, 1] = np.inf
    q[2, 0, 0, 1] = 7
    scores, pairs = best_ref(q)
    assert pairs.tolist() == [[5, 4, -1], [-1, -1, -1]]
    assert np.isinf(scores[0, 0]) and scores[0, 1] == 7 and np.isnan(scores[0, 2]) and np.isnan(scores[1]).all()
    assert (pair_keys(q)[:, 1, :] == NO_KEY).all()
    recs = detect_ref(q, 8, 0, 0, (10, 20, 3, 2, 1, 1), base=3)
    assert recs["tmpl_idx"].tolist() == [5, 5] and recs["score"].tolist() == [7, np.inf]
    assert recs["transform"][:, 2].tolist() == [11, 10] and recs["transform"][:, 5].tolist() == [20, 20]
    scores, pairs = best_ref(np.zeros((0, 1, 2, 2), dtype=np.float32))
    assert np.isnan(scores).all() and np.all(pairs == -1)
