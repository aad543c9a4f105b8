"""Checks of the calls by matched fraction (include/fdcm.h, "Detections by matched fraction") that need no scene: the library
exports the entry points, the binding and the header know them, and every argument check returns FDCM_EINVAL with its own
message before any handle or device is touched (the handles are NULL throughout: a late check would report them instead)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

EINVAL = -1
f32 = np.float32
NEW_SYMBOLS = ["fdcm_search_exhaustive_detect_all_matched", "fdcm_matched_fractions", "fdcm_templates_matched_totals"]
SUBNORMAL = float(np.array([1], dtype=np.uint32).view(np.float32)[0])


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def _all(capi, rot=None, grid=(0, 0, 4, 4, 1, 1), max_score=1.0, max_det=8, permille=300, margin=0, penalty=-1, tau=1.0,
         min_matched=0.5, out=True, n_out=True, boxes=False, matched=False):
    o, n = C.c_void_p(), C.c_int64()
    b = np.zeros(4 * 4096, dtype=np.int32)
    m = np.zeros(4096, dtype=np.float32)
    g = capi.Grid(*grid) if grid is not None else None
    return capi.lib().fdcm_search_exhaustive_detect_all_matched(
        None, None, C.byref(rot) if rot is not None else None, C.byref(g) if g is not None else None, max_score, max_det, permille,
        margin, penalty, tau, min_matched, 0, C.byref(o) if out else None, C.byref(n) if n_out else None,
        b.ctypes.data_as(C.POINTER(C.c_int32)) if boxes else None, capi.fptr(m) if matched else None)


def _fractions(capi, poses, rot=None, n=None, out=True):
    p = np.ascontiguousarray(poses, dtype=np.int32).reshape(-1, 4)
    fr = np.zeros(max(1, len(p)), dtype=np.float32)
    return capi.lib().fdcm_matched_fractions(None, None, C.byref(rot) if rot is not None else None,
                                             p.ctypes.data_as(C.POINTER(C.c_int32)) if len(p) else None, len(p) if n is None else n,
                                             capi.fptr(fr) if out else None)


def test_exports_and_binds_the_entry_points(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in bound
    args = bound["fdcm_search_exhaustive_detect_all_matched"][2]
    assert len(args) == 16 and args[4] is C.c_float and args[10] is C.c_float and args[11] is C.c_int32
    assert len(bound["fdcm_matched_fractions"][2]) == 6 and len(bound["fdcm_templates_matched_totals"][2]) == 2
    # the call it extends keeps its binding
    assert len(bound["fdcm_search_exhaustive_detect_all"][2]) == 14
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    p = inspect.signature(fd.exhaustive_detect_all).parameters
    assert list(p)[:3] == ["featuremap", "templates", "max_score"]
    assert p["min_matched"].default is None and p["return_matched"].default is False and p["return_boxes"].default is False
    assert p["overlap"].default == 0.3 and p["max_detections"].default == 1024 and p["line_caps"].default is None
    p = inspect.signature(fd.matched_fractions).parameters
    assert list(p) == ["featuremap", "templates", "poses", "angles", "pivot", "line_caps"]
    assert p["angles"].default is None and p["pivot"].default == "center" and p["line_caps"].default is None
    p = inspect.signature(DeviceFeatureMap.exhaustive_detect_all).parameters
    assert p["min_matched"].default is None and p["matched"].default is False and p["boxes"].default is False
    assert list(inspect.signature(DeviceFeatureMap.matched_fractions).parameters) == ["self", "templates", "poses", "cs", "pivots"]
    assert callable(DeviceTemplates.matched_totals)
    with open(os.path.join(os.path.dirname(capi.LIB_PATH), "..", "include", "fdcm.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert "int " + name + "(" in header
    assert "Detections by matched fraction" in header and "tests/matched_ref.py" in header
    assert "only that pair" in header  # the limitation is stated
    with open(os.path.join(os.path.dirname(capi.LIB_PATH), "csrc", "fdcm_internal.h")) as f:
        assert "FDCM_MATCHED_FLAT" in f.read()


def test_valid_arguments_reach_the_handles(capi):
    """The bounds are inclusive: with them the calls go on to the (null) handles."""
    for mm in (0.0, -0.0, SUBNORMAL, 0.5, float(np.nextafter(f32(1), f32(0))), 1.0):
        for ms, md in [(0.0, 1), (np.inf, 4096)]:
            assert _all(capi, max_score=ms, max_det=md, min_matched=mm, boxes=True, matched=True) == EINVAL
            assert "null featuremap/templates" in _err(capi)
    assert _all(capi, min_matched=0.3) == EINVAL and "null featuremap/templates" in _err(capi)  # both arrays may be null
    lim = (1 << 24) - 1
    assert _fractions(capi, [[0, 0, lim, -lim], [7, 0, 0, 0]]) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _fractions(capi, np.zeros((0, 4)), out=False) == EINVAL and "null featuremap/templates" in _err(capi)  # n = 0: no array
    cs = np.float32([[1, 0], [0, 1]])
    assert _fractions(capi, [[0, 1, 3, 4]], rot=capi.Rotations(capi.fptr(cs), 2, None)) == EINVAL
    assert "null featuremap/templates" in _err(capi)


@pytest.mark.parametrize("min_matched", [np.nan, -1.0, -SUBNORMAL, -np.inf, float(np.nextafter(f32(1), f32(2))), 2.0, np.inf])
def test_bad_min_matched_is_einval(capi, min_matched):
    assert _all(capi, min_matched=min_matched) == EINVAL and "min_matched must be in [0, 1]" in _err(capi)


def test_what_the_threshold_call_rejects_is_einval(capi):
    for ms in (np.nan, -1.0, -SUBNORMAL):
        assert _all(capi, max_score=ms) == EINVAL and "max_score must be >= 0" in _err(capi)
    for md in (0, 4097, -1):
        assert _all(capi, max_det=md) == EINVAL and "max_detections must be in [1, 4096]" in _err(capi)
    for permille in (-1, 1001):
        assert _all(capi, permille=permille) == EINVAL and "overlap_permille must be in [0, 1000]" in _err(capi)
    for margin in (-1, 4097):
        assert _all(capi, margin=margin) == EINVAL and "margin must be in [0, 4096]" in _err(capi)
    assert _all(capi, out=False) == EINVAL and "null output" in _err(capi)
    assert _all(capi, n_out=False) == EINVAL and "null output" in _err(capi)
    assert _all(capi, grid=None) == EINVAL and "grid is null" in _err(capi)
    for grid, what in [((0, 0, 4, 4, 0, 1), "stride"), ((0, 0, 0, 4, 1, 1), "nx and ny"), ((0, 0, (1 << 13) + 1, 1 << 13, 1, 1), "2^26")]:
        assert _all(capi, grid=grid) == EINVAL and what in _err(capi)
    for penalty in (-2, 2):
        assert _all(capi, penalty=penalty) == EINVAL and "unknown penalty" in _err(capi)
    for tau in (np.nan, np.inf):
        assert _all(capi, penalty=1, tau=tau) == EINVAL and "tau must be finite" in _err(capi)
    cs = np.float32([[1, 0], [np.nan, 0]])
    assert _all(capi, rot=capi.Rotations(capi.fptr(cs), 2, None)) == EINVAL and "c and s must be finite" in _err(capi)
    assert _all(capi, rot=capi.Rotations(None, 3, None)) == EINVAL and "cs is null" in _err(capi)


def test_what_the_pose_call_rejects_is_einval(capi):
    assert _fractions(capi, [[0, 0, 0, 0]], n=-1) == EINVAL and "n is negative" in _err(capi)
    assert _fractions(capi, np.zeros((0, 4)), n=2) == EINVAL and "poses is null" in _err(capi)
    assert _fractions(capi, [[0, 0, 0, 0]], out=False) == EINVAL and "fractions is null" in _err(capi)
    assert _fractions(capi, [[-1, 0, 0, 0]]) == EINVAL and "tmpl is outside the template set" in _err(capi)
    assert _fractions(capi, [[0, 1, 0, 0]]) == EINVAL and "a must be 0 without rotations" in _err(capi)
    assert _fractions(capi, [[0, -1, 0, 0]]) == EINVAL and "a must be 0 without rotations" in _err(capi)
    cs = np.float32([[1, 0], [0, 1]])
    rot = capi.Rotations(capi.fptr(cs), 2, None)
    assert _fractions(capi, [[0, 2, 0, 0]], rot=rot) == EINVAL and "a must be in [0, n - 1]" in _err(capi)
    for x, y in [(1 << 24, 0), (0, -(1 << 24))]:
        assert _fractions(capi, [[0, 0, x, y]]) == EINVAL and "|t| < 2^24" in _err(capi)
    bad = np.float32([[1, 0], [np.inf, 0]])
    assert _fractions(capi, [[0, 0, 0, 0]], rot=capi.Rotations(capi.fptr(bad), 2, None)) == EINVAL and "c and s must be finite" in _err(capi)
    assert _fractions(capi, [[0, 0, 0, 0]], rot=capi.Rotations(None, 3, None)) == EINVAL and "cs is null" in _err(capi)
    t = np.zeros(3, dtype=np.float32)
    assert capi.lib().fdcm_templates_matched_totals(None, capi.fptr(t)) == EINVAL and "templates is null" in _err(capi)
