"""CPU-only checks of the gate inside the minimum (include/fdcm.h, "Gate inside the minimum"): the library exports the three
entry points, the binding knows their prototypes, the header declares them, every argument check of their siblings and the
check of `gate` return FDCM_EINVAL with a message before any handle or device is touched (the handles are null here: a check
that came late would report "null featuremap/templates"), and the Python signatures keep every existing default and carry
gate="winner".  The empty inputs and everything with a device: test_gpu_gate.py."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

EINVAL = -1
INF = float("inf")
NEW_SYMBOLS = ("fdcm_best_map_gated", "fdcm_search_exhaustive_detect_all_gated", "fdcm_search_exhaustive_detect_windows_gated")
GOOD = (0, 0, 1, -4, -4, 9, 9)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def _dense(capi, rot=None, grid=(0, 0, 4, 4, 1, 1), max_score=1.0, max_det=8, permille=300, margin=0, penalty=-1, tau=1.0,
           min_matched=0.5, gate=1, out=True, n_out=True):
    o, n = C.c_void_p(), C.c_int64()
    g = capi.Grid(*grid) if grid is not None else None
    return capi.lib().fdcm_search_exhaustive_detect_all_gated(
        None, None, C.byref(rot) if rot is not None else None, C.byref(g) if g is not None else None, max_score, max_det, permille,
        margin, penalty, tau, min_matched, gate, 0, C.byref(o) if out else None, C.byref(n) if n_out else None, None, None)


def _windows(capi, jobs, rot=None, sx=1, sy=1, wrap=0, max_score=INF, max_det=100, permille=300, margin=0, penalty=0, tau=1.0,
             min_matched=0.5, gate=1, n_jobs=None, out=True, n_out=True):
    jobs = None if jobs is None else np.ascontiguousarray(np.asarray(jobs, dtype=np.int32).reshape(-1, 7))
    o, n = C.c_void_p(), C.c_int64()
    return capi.lib().fdcm_search_exhaustive_detect_windows_gated(
        None, None, C.byref(rot) if rot is not None else None,
        jobs.ctypes.data_as(C.POINTER(capi.PoseWindow)) if jobs is not None else None,
        (0 if jobs is None else jobs.shape[0]) if n_jobs is None else n_jobs, sx, sy, wrap, max_score, max_det, permille, margin, penalty,
        tau, min_matched, gate, 0, C.byref(o) if out else None, C.byref(n) if n_out else None, None, None, None)


def _map(capi, rot=None, grid=(0, 0, 4, 4, 1, 1), penalty=-1, tau=1.0, min_matched=0.5, planes=(True, True, True)):
    g = capi.Grid(*grid) if grid is not None else None
    s, p, m = np.zeros(16, dtype=np.float32), np.zeros(16, dtype=np.int32), np.zeros(16, dtype=np.float32)
    return capi.lib().fdcm_best_map_gated(None, None, C.byref(rot) if rot is not None else None, C.byref(g) if g is not None else None,
                                          penalty, tau, min_matched, capi.fptr(s) if planes[0] else None,
                                          p.ctypes.data_as(C.POINTER(C.c_int32)) if planes[1] else None, capi.fptr(m) if planes[2] else None)


def test_exports_binds_and_declares(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    with open(os.path.join(os.path.dirname(capi.LIB_PATH), "..", "include", "fdcm.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in bound and bound[name][1] is C.c_int
        assert "int " + name + "(" in header
    args = bound["fdcm_best_map_gated"][2]
    assert len(args) == 10 and args[6] is C.c_float and args[9] == C.POINTER(C.c_float)
    args = bound["fdcm_search_exhaustive_detect_all_gated"][2]
    assert len(args) == 17 and args[10] is C.c_float and args[11] is C.c_int and args[12] is C.c_int32
    args = bound["fdcm_search_exhaustive_detect_windows_gated"][2]
    assert len(args) == 22 and args[14] is C.c_float and args[15] is C.c_int and args[16] is C.c_int32
    # the calls they extend keep their bindings
    assert len(bound["fdcm_best_map"][2]) == 8 and len(bound["fdcm_search_exhaustive_detect_all_matched"][2]) == 16
    assert len(bound["fdcm_search_exhaustive_detect_windows"][2]) == 21
    assert "#define FDCM_GATE_WINNER 0" in header and "#define FDCM_GATE_ALL 1" in header
    assert (capi.GATE_WINNER, capi.GATE_ALL) == (0, 1)
    assert "Gate inside the minimum" in header and "tests/gate_ref.py" in header
    assert "only that pair" in header and header.count("lifts this limitation") == 2


def test_valid_arguments_reach_the_null_handles(capi):
    for gate in (0, 1):
        for mm in (0.0, 0.5, 1.0):
            assert _dense(capi, gate=gate, min_matched=mm) == EINVAL and "null featuremap/templates" in _err(capi)
            assert _windows(capi, [GOOD], gate=gate, min_matched=mm) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _dense(capi, max_score=INF, max_det=4096, permille=1000, margin=4096, penalty=1, tau=1.5) == EINVAL
    assert "null featuremap/templates" in _err(capi)
    assert _windows(capi, None, n_jobs=0) == EINVAL and "null featuremap/templates" in _err(capi)
    for planes in [(True, True, True), (True, False, False), (False, True, False), (False, False, True)]:
        for mm in (0.0, 1.0):
            assert _map(capi, min_matched=mm, planes=planes) == EINVAL and "null featuremap/templates" in _err(capi)


@pytest.mark.parametrize("gate", [-1, 2, 3, 1 << 30])
def test_gate_outside_0_and_1_is_einval(capi, gate):
    assert _dense(capi, gate=gate) == EINVAL and "gate must be FDCM_GATE_WINNER or FDCM_GATE_ALL" in _err(capi)
    assert _windows(capi, [GOOD], gate=gate) == EINVAL and "gate must be FDCM_GATE_WINNER or FDCM_GATE_ALL" in _err(capi)


@pytest.mark.parametrize("gate", [0, 1])
def test_what_the_dense_sibling_rejects(capi, gate):
    d = lambda **kw: _dense(capi, gate=gate, **kw)
    for mm in (np.nan, -1.0, 2.0, float(np.nextafter(np.float32(1), np.float32(2)))):
        assert d(min_matched=mm) == EINVAL and "min_matched must be in [0, 1]" in _err(capi)
    for ms in (np.nan, -1.0):
        assert d(max_score=ms) == EINVAL and "max_score must be >= 0" in _err(capi)
    for md in (0, 4097, -1):
        assert d(max_det=md) == EINVAL and "max_detections must be in [1, 4096]" in _err(capi)
    for permille in (-1, 1001):
        assert d(permille=permille) == EINVAL and "overlap_permille must be in [0, 1000]" in _err(capi)
    for margin in (-1, 4097):
        assert d(margin=margin) == EINVAL and "margin must be in [0, 4096]" in _err(capi)
    assert d(out=False) == EINVAL and "null output" in _err(capi)
    assert d(n_out=False) == EINVAL and "null output" in _err(capi)
    assert d(grid=None) == EINVAL and "grid is null" in _err(capi)
    for grid, what in [((0, 0, 4, 4, 0, 1), "stride"), ((0, 0, 0, 4, 1, 1), "nx and ny"), ((0, 0, (1 << 13) + 1, 1 << 13, 1, 1), "2^26")]:
        assert d(grid=grid) == EINVAL and what in _err(capi)
    for penalty in (-2, 2):
        assert d(penalty=penalty) == EINVAL and "unknown penalty" in _err(capi)
    for tau in (np.nan, np.inf):
        assert d(penalty=1, tau=tau) == EINVAL and "tau must be finite" in _err(capi)
    cs = np.float32([[1, 0], [np.nan, 0]])
    assert d(rot=capi.Rotations(capi.fptr(cs), 2, None)) == EINVAL and "c and s must be finite" in _err(capi)
    assert d(rot=capi.Rotations(None, 3, None)) == EINVAL and "cs is null" in _err(capi)


def test_what_the_best_map_rejects(capi):
    assert _map(capi, planes=(False, False, False)) == EINVAL and "are all null" in _err(capi)
    for mm in (np.nan, -0.5, 1.5):
        assert _map(capi, min_matched=mm) == EINVAL and "min_matched must be in [0, 1]" in _err(capi)
    assert _map(capi, grid=None) == EINVAL and "grid is null" in _err(capi)
    for grid, what in [((0, 0, 4, 4, 1, 0), "stride"), ((0, 0, 4, 0, 1, 1), "nx and ny"), ((0, 0, (1 << 13) + 1, 1 << 13, 1, 1), "2^26")]:
        assert _map(capi, grid=grid) == EINVAL and what in _err(capi)
    assert _map(capi, penalty=3) == EINVAL and "unknown penalty" in _err(capi)
    assert _map(capi, penalty=1, tau=np.nan) == EINVAL and "tau must be finite" in _err(capi)
    assert _map(capi, rot=capi.Rotations(None, 3, None)) == EINVAL and "cs is null" in _err(capi)


@pytest.mark.parametrize("gate", [0, 1])
def test_what_the_windows_sibling_rejects(capi, gate):
    w = lambda jobs=(GOOD,), **kw: _windows(capi, list(jobs) if jobs is not None else None, gate=gate, **kw)
    for kw, what in [
        (dict(max_score=float("nan")), "max_score must be >= 0"), (dict(max_score=-1.0), "max_score must be >= 0"),
        (dict(max_det=0), "max_detections must be in [1, 4096]"), (dict(max_det=4097), "max_detections must be in [1, 4096]"),
        (dict(permille=-1), "overlap_permille must be in [0, 1000]"), (dict(permille=1001), "overlap_permille must be in [0, 1000]"),
        (dict(margin=-1), "margin must be in [0, 4096]"), (dict(margin=4097), "margin must be in [0, 4096]"),
        (dict(penalty=2), "unknown penalty"), (dict(tau=float("inf")), "tau must be finite"),
        (dict(min_matched=float("nan")), "min_matched must be in [0, 1]"), (dict(min_matched=1.5), "min_matched must be in [0, 1]"),
        (dict(sx=0), "strides sx and sy must be >= 1"), (dict(sy=-1), "strides sx and sy must be >= 1"),
        (dict(wrap=2), "wrap must be 0 or 1"), (dict(out=False), "null output"), (dict(n_out=False), "null output"),
        (dict(n_jobs=-1), "n_jobs is negative"), (dict(n_jobs=(1 << 22) + 1), "n_jobs must be at most 2^22"),
    ]:
        assert w(**kw) == EINVAL and what in _err(capi), kw
    assert w(jobs=None, n_jobs=1) == EINVAL and "jobs is null" in _err(capi)
    cs4 = np.tile(np.float32([[1, 0]]), (4, 1))
    rot = capi.Rotations(capi.fptr(cs4), 4, None)
    for job, wrap, what in [
        ((-1, 0, 1, 0, 0, 3, 3), 0, "tmpl is outside the template set"), ((0, 0, 0, 0, 0, 3, 3), 0, "na must be in [1, n]"),
        ((0, 4, 1, 0, 0, 3, 3), 1, "a0 must be in [0, n - 1]"), ((0, 3, 2, 0, 0, 3, 3), 0, "a0 + na must be at most n without wrap"),
        ((0, 0, 1, 0, 0, 0, 3), 0, "nx and ny must be >= 1"), ((0, 0, 1, 0, 0, 257, 256), 0, "na * nx * ny must be at most 65536"),
        ((0, 0, 1, -(1 << 24), 0, 3, 3), 0, "|t| < 2^24"),
    ]:
        assert w(jobs=[(0, 0, 1, 0, 0, 3, 3), job], rot=rot, wrap=wrap) == EINVAL and what in _err(capi), job
    assert w(jobs=[(0, 1, 1, 0, 0, 3, 3)]) == EINVAL and "a0 must be in [0, n - 1]" in _err(capi)  # translations only
    bad = np.float32([[1, 0], [np.nan, 0]])
    assert w(rot=capi.Rotations(capi.fptr(bad), 2, None)) == EINVAL and "c and s must be finite" in _err(capi)
    assert w(rot=capi.Rotations(None, 2, None)) == EINVAL and "cs is null" in _err(capi)


def test_python_signatures_keep_their_defaults_and_carry_the_gate(capi):
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap
    p = inspect.signature(fd.exhaustive_detect_all).parameters
    assert list(p)[:3] == ["featuremap", "templates", "max_score"] and list(p)[-1] == "gate" and p["gate"].default == "winner"
    assert p["min_matched"].default is None and p["return_matched"].default is False and p["return_boxes"].default is False
    assert p["overlap"].default == 0.3 and p["max_detections"].default == 1024 and p["line_caps"].default is None
    p = inspect.signature(fd.exhaustive_detect_windows).parameters
    assert list(p)[:4] == ["featuremap", "templates", "jobs", "max_score"] and list(p)[-1] == "gate" and p["gate"].default == "winner"
    assert p["min_matched"].default is None and p["return_jobs"].default is False and p["wrap"].default is False
    p = inspect.signature(fd.exhaustive_detect_refined).parameters
    assert list(p)[:9] == ["featuremap", "templates", "max_score", "coarse_angles", "fine_angles", "coarse_stride", "half_angles", "half_x",
                           "half_y"]
    assert list(p)[-1] == "gate" and p["gate"].default == "winner" and p["coarse_overlap"].default == 1.0
    p = inspect.signature(fd.best_score_map).parameters
    assert list(p) == ["featuremap", "templates", "stride", "penalty", "angles", "pivot", "window", "line_caps", "min_matched",
                       "return_matched"]
    assert p["min_matched"].default is None and p["return_matched"].default is False and p["stride"].default == 1
    p = inspect.signature(DeviceFeatureMap.exhaustive_detect_all).parameters
    assert list(p)[-1] == "gate" and p["gate"].default == "winner" and p["min_matched"].default is None and p["matched"].default is False
    p = inspect.signature(DeviceFeatureMap.exhaustive_detect_windows).parameters
    assert list(p)[-1] == "gate" and p["gate"].default == "winner" and p["job_index"].default is False
    p = inspect.signature(DeviceFeatureMap.best_map).parameters
    assert list(p) == ["self", "templates", "grid", "cs", "pivots", "penalty", "tau", "min_matched", "matched"]
    assert p["min_matched"].default is None and p["matched"].default is False
    # the gate is checked before anything else is looked at
    for call in (fd.exhaustive_detect_all, fd.exhaustive_detect_windows, fd.exhaustive_detect_refined):
        with pytest.raises(ValueError, match="gate must be"):
            call(None, None, *([None] * (8 if call is fd.exhaustive_detect_refined else 2)), gate="best")
    for method in (DeviceFeatureMap.exhaustive_detect_all, DeviceFeatureMap.exhaustive_detect_windows):
        with pytest.raises(ValueError, match="gate must be"):
            method(None, None, None, gate=1)
