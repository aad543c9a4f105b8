"""CPU-only checks of the detections suppressed by footprint overlap (include/fdcm.h, "Detections suppressed by footprint
overlap"): the library exports the entry points and the binding knows them, and every argument check returns FDCM_EINVAL
with a message before any handle or device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

EINVAL = -1
NEW_SYMBOLS = ["fdcm_search_exhaustive_detect_nms", "fdcm_templates_footprints", "fdcm_lines_footprints"]


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


def _nms(capi, rot=None, grid=(0, 0, 4, 4, 1, 1), k=1, permille=300, margin=0, penalty=-1, tau=1.0, out=True, n_out=True, boxes=False):
    o, n = C.c_void_p(), C.c_int64()
    b = np.zeros(4 * 64, dtype=np.int32)
    g = capi.Grid(*grid) if grid is not None else None
    return capi.lib().fdcm_search_exhaustive_detect_nms(
        None, None, C.byref(rot) if rot is not None else None, C.byref(g) if g is not None else None, k, permille, margin, penalty,
        tau, 0, C.byref(o) if out else None, b.ctypes.data_as(C.POINTER(C.c_int32)) if boxes else None, C.byref(n) if n_out else None)


def test_exports_and_binds_the_entry_points(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0] for s in capi.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in bound
    import inspect
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    for f in (DeviceFeatureMap.exhaustive_detect_nms, DeviceTemplates.footprints, fd.exhaustive_detect_nms, fd.template_footprints):
        assert callable(f)
    p = inspect.signature(fd.exhaustive_detect_nms).parameters
    assert p["overlap"].default == 0.3 and p["k"].default == 8 and p["margin"].default == 0 and p["return_boxes"].default is False
    p = inspect.signature(DeviceFeatureMap.exhaustive_detect_nms).parameters
    assert p["overlap_permille"].default == 300 and p["boxes"].default is False
    with open(os.path.join(os.path.dirname(capi.LIB_PATH), "..", "include", "fdcm.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert "int " + name + "(" in header


def test_valid_arguments_reach_the_handles(capi):
    """The bounds are inclusive: with them the call goes on to the (null) handles."""
    for permille, margin, k in [(0, 0, 1), (1000, 4096, 64), (300, 3, 8)]:
        assert _nms(capi, k=k, permille=permille, margin=margin, boxes=True) == EINVAL
        assert "null featuremap/templates" in _err(capi)


@pytest.mark.parametrize("permille", [-1, 1001, -1000, 1 << 30])
def test_overlap_out_of_range_is_einval(capi, permille):
    assert _nms(capi, permille=permille) == EINVAL and "overlap_permille must be in [0, 1000]" in _err(capi)


@pytest.mark.parametrize("margin", [-1, 4097, 1 << 30])
def test_margin_out_of_range_is_einval(capi, margin):
    assert _nms(capi, margin=margin) == EINVAL and "margin must be in [0, 4096]" in _err(capi)
    b = np.zeros(4, dtype=np.int32)
    assert capi.lib().fdcm_templates_footprints(None, None, margin, b.ctypes.data_as(C.POINTER(C.c_int32))) == EINVAL
    assert "margin must be in [0, 4096]" in _err(capi)
    assert capi.lib().fdcm_lines_footprints(None, None, 0, None, margin, None) == EINVAL and "margin must be in [0, 4096]" in _err(capi)


@pytest.mark.parametrize("k", [0, 65, -1])
def test_k_out_of_range_is_einval(capi, k):
    assert _nms(capi, k=k) == EINVAL and "k must be in [1, 64]" in _err(capi)


def test_null_pointers_are_einval(capi):
    assert _nms(capi, out=False) == EINVAL and "null output" in _err(capi)
    assert _nms(capi, n_out=False) == EINVAL and "null output" in _err(capi)
    assert _nms(capi, grid=None) == EINVAL and "grid is null" in _err(capi)
    assert _nms(capi) == EINVAL and "null featuremap/templates" in _err(capi)  # rot and boxes_out may be null, the handles not
    b = np.zeros(4, dtype=np.int32)
    assert capi.lib().fdcm_templates_footprints(None, None, 0, b.ctypes.data_as(C.POINTER(C.c_int32))) == EINVAL
    assert "templates is null" in _err(capi)


@pytest.mark.parametrize("grid,what", [
    ((0, 0, 4, 4, 0, 1), "stride"), ((0, 0, 4, 4, 1, -2), "stride"), ((0, 0, 0, 4, 1, 1), "nx and ny"), ((0, 0, 4, -1, 1, 1), "nx and ny"),
    ((0, 0, 1 << 16, 1 << 15, 1, 1), "2^26"), ((0, 0, (1 << 13) + 1, 1 << 13, 1, 1), "2^26"), ((0, 0, (1 << 26) + 1, 1, 1, 1), "2^26"),
])
def test_bad_grids_are_einval(capi, grid, what):
    assert _nms(capi, grid=grid) == EINVAL and what in _err(capi)


def test_grid_of_2_26_points_passes_the_grid_checks(capi):
    for g in [(0, 0, 1 << 13, 1 << 13, 1, 1), (-5, 7, 1 << 26, 1, 1, 1)]:
        assert _nms(capi, grid=g) == EINVAL and "null featuremap/templates" in _err(capi)


@pytest.mark.parametrize("penalty", [-2, 2, 7])
def test_unknown_penalty_is_einval(capi, penalty):
    assert _nms(capi, penalty=penalty) == EINVAL and "unknown penalty" in _err(capi)


@pytest.mark.parametrize("tau", [np.nan, np.inf, -np.inf])
def test_tau_not_finite_is_einval(capi, tau):
    for penalty in (-1, capi.DEFAULT_PENALTY, capi.EXPONENTIAL_PENALTY):
        assert _nms(capi, penalty=penalty, tau=tau) == EINVAL and "tau must be finite" in _err(capi)


def test_rotation_checks_are_einval(capi):
    """What the rotation call rejects about a table, when there is one; checked before the handles (null here)."""
    b = np.zeros(64, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    lines, off = np.zeros((1, 4), dtype=np.float32), np.int64([0, 1])
    for cs, what in [(np.zeros((0, 2)), "n must be >= 1"), ([[1, 0], [np.nan, 0]], "c and s must be finite"),
                     ([[1, np.inf]], "c and s must be finite")]:
        r, keep = _rot(capi, cs)
        assert _nms(capi, rot=r) == EINVAL and what in _err(capi)
        assert capi.lib().fdcm_templates_footprints(None, C.byref(r), 0, b) == EINVAL and what in _err(capi)
        assert capi.lib().fdcm_lines_footprints(capi.fptr(lines), off.ctypes.data_as(C.POINTER(C.c_int64)), 1, C.byref(r), 0, b) == EINVAL
        assert what in _err(capi)
    r = capi.Rotations(None, 3, None)
    assert _nms(capi, rot=r) == EINVAL and "cs is null" in _err(capi)


def test_lines_footprints_checks_its_arguments(capi):
    b = np.zeros(64, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    lines = np.zeros((2, 4), dtype=np.float32)
    off = lambda *v: np.array(v, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    f = capi.lib().fdcm_lines_footprints
    assert f(capi.fptr(lines), None, 2, None, 0, b) == EINVAL and "bad offsets" in _err(capi)
    assert f(capi.fptr(lines), off(0, 1), -1, None, 0, b) == EINVAL and "bad offsets" in _err(capi)
    assert f(capi.fptr(lines), off(1, 2), 1, None, 0, b) == EINVAL and "offsets[0] must be 0" in _err(capi)
    assert f(capi.fptr(lines), off(0, 2, 1), 2, None, 0, b) == EINVAL and "ascending" in _err(capi)
    assert f(None, off(0, 2), 1, None, 0, b) == EINVAL and "lines is null" in _err(capi)
    assert f(capi.fptr(lines), off(0, 2), 1, None, 0, None) == EINVAL and "boxes_out is null" in _err(capi)
    cs = np.float32([[1, 0]])
    piv = np.float32([[0, np.nan]])
    r = capi.Rotations(capi.fptr(cs), 1, capi.fptr(piv))
    assert f(capi.fptr(lines), off(0, 2), 1, C.byref(r), 0, b) == EINVAL and "pivots must be finite" in _err(capi)
    assert f(None, None, 0, None, 0, None) == 0  # no templates: nothing to write
    assert f(capi.fptr(lines), off(0, 2), 1, None, 0, b) == 0
