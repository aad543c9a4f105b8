"""CPU-only checks of the calls with objects (include/fdcm.h, "Objects"), in the manner of test_gate_abi.py: the library exports
the three entry points, the binding knows their prototypes, the header declares them, every argument check that can be
reached without a handle returns FDCM_EINVAL with a message before any handle or device is touched (the handles are null
here: a check that came late would report "null featuremap/templates"), the Python functions have the documented signatures,
and the functions that were there keep theirs.  The labels against a real set, the bound on the planes with real handles and
everything with a device: test_gpu_objects.py."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

EINVAL = -1
INF = float("inf")
NEW_SYMBOLS = ("fdcm_best_map_objects", "fdcm_search_exhaustive_detect_objects", "fdcm_search_exhaustive_detect_windows_objects")
GOOD = (0, 0, 1, -4, -4, 9, 9)
I32P = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def _floats(capi, v):
    if v is None:
        return None, None
    a = np.ascontiguousarray(v, dtype=np.float32)
    return a, capi.fptr(a)


def _dense(capi, rot=None, grid=(0, 0, 4, 4, 1, 1), G=2, max_score=(1.0, INF), min_matched=(0.5, 0.0), max_det=8, permille=300,
           cross=600, margin=0, penalty=-1, tau=1.0, gate=1, out=True, n_out=True):
    o, n = C.c_void_p(), C.c_int64()
    g = capi.Grid(*grid) if grid is not None else None
    obj = np.zeros(4, dtype=np.int32)
    ms, msp = _floats(capi, max_score)
    mm, mmp = _floats(capi, min_matched)
    return capi.lib().fdcm_search_exhaustive_detect_objects(
        None, None, C.byref(rot) if rot is not None else None, C.byref(g) if g is not None else None, obj.ctypes.data_as(I32P), G, msp, mmp,
        max_det, permille, cross, margin, penalty, tau, gate, 0, C.byref(o) if out else None, C.byref(n) if n_out else None, None, None)


def _windows(capi, jobs, rot=None, sx=1, sy=1, wrap=0, G=2, max_score=(1.0, INF), min_matched=(0.5, 0.0), max_det=100, permille=300,
             cross=600, margin=0, penalty=0, tau=1.0, gate=1, n_jobs=None, out=True, n_out=True):
    jobs = None if jobs is None else np.ascontiguousarray(np.asarray(jobs, dtype=np.int32).reshape(-1, 7))
    o, n = C.c_void_p(), C.c_int64()
    obj = np.zeros(4, dtype=np.int32)
    ms, msp = _floats(capi, max_score)
    mm, mmp = _floats(capi, min_matched)
    return capi.lib().fdcm_search_exhaustive_detect_windows_objects(
        None, None, C.byref(rot) if rot is not None else None, jobs.ctypes.data_as(C.POINTER(capi.PoseWindow)) if jobs is not None else None,
        (0 if jobs is None else jobs.shape[0]) if n_jobs is None else n_jobs, sx, sy, wrap, obj.ctypes.data_as(I32P), G, msp, mmp, max_det,
        permille, cross, margin, penalty, tau, gate, 0, C.byref(o) if out else None, C.byref(n) if n_out else None, None, None, None)


def _map(capi, rot=None, grid=(0, 0, 4, 4, 1, 1), G=2, penalty=-1, tau=1.0, min_matched=(0.5, 0.0), planes=(True, True, True)):
    g = capi.Grid(*grid) if grid is not None else None
    s, p, m = np.zeros(32, dtype=np.float32), np.zeros(32, dtype=np.int32), np.zeros(32, dtype=np.float32)
    obj = np.zeros(4, dtype=np.int32)
    mm, mmp = _floats(capi, min_matched)
    return capi.lib().fdcm_best_map_objects(None, None, C.byref(rot) if rot is not None else None, C.byref(g) if g is not None else None,
                                            penalty, tau, obj.ctypes.data_as(I32P), G, mmp, capi.fptr(s) if planes[0] else None,
                                            p.ctypes.data_as(I32P) if planes[1] else None, capi.fptr(m) if planes[2] else None)


def test_exports_binds_and_declares(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    with open(os.path.join(os.path.dirname(capi.LIB_PATH), "..", "include", "fdcm.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in bound and bound[name][1] is C.c_int
        assert "int " + name + "(" in header
    args = bound["fdcm_best_map_objects"][2]
    assert len(args) == 12 and args[6] == I32P and args[7] is C.c_int32 and args[8] == C.POINTER(C.c_float)
    args = bound["fdcm_search_exhaustive_detect_objects"][2]
    assert len(args) == 20 and args[4] == I32P and args[5] is C.c_int32 and args[6] == args[7] == C.POINTER(C.c_float)
    assert args[10] is C.c_int32 and args[14] is C.c_int and args[15] is C.c_int32
    args = bound["fdcm_search_exhaustive_detect_windows_objects"][2]
    assert len(args) == 25 and args[8] == I32P and args[9] is C.c_int32 and args[10] == args[11] == C.POINTER(C.c_float)
    assert args[14] is C.c_int32 and args[18] is C.c_int and args[24] == I32P
    # the calls they stand beside keep their bindings
    assert len(bound["fdcm_best_map_gated"][2]) == 10 and len(bound["fdcm_search_exhaustive_detect_all_gated"][2]) == 17
    assert len(bound["fdcm_search_exhaustive_detect_windows_gated"][2]) == 22
    assert "/* Objects:" in header and "tests/objects_ref.py" in header and "cross_permille" in header
    assert "n_objects * nx * ny > 2^26" in header and "key(g, o) = (bits of q, g, u)" in header


def test_valid_arguments_reach_the_null_handles(capi):
    for gate in (0, 1):
        for mm in ((0.0, 0.0), (0.5, 1.0), None):
            assert _dense(capi, gate=gate, min_matched=mm) == EINVAL and "null featuremap/templates" in _err(capi)
            assert _windows(capi, [GOOD], gate=gate, min_matched=mm) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _dense(capi, G=256, max_score=[INF] * 256, min_matched=None, max_det=4096, permille=1000, cross=1000, margin=4096, penalty=1,
                  tau=1.5) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _dense(capi, G=1, max_score=[0.0], min_matched=[1.0], cross=0, permille=0) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _windows(capi, None, n_jobs=0) == EINVAL and "null featuremap/templates" in _err(capi)
    for planes in [(True, True, True), (True, False, False), (False, True, False), (False, False, True)]:
        for mm in ((0.0, 1.0), None):
            assert _map(capi, min_matched=mm, planes=planes) == EINVAL and "null featuremap/templates" in _err(capi)
    # 2 objects on a grid of 2^25 points: exactly the bound
    assert _dense(capi, grid=(0, 0, 1 << 13, 1 << 12, 1, 1)) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _map(capi, grid=(0, 0, 1 << 13, 1 << 12, 1, 1)) == EINVAL and "null featuremap/templates" in _err(capi)


@pytest.mark.parametrize("call", ["dense", "windows"])
def test_what_the_objects_add(capi, call):
    f = (lambda **kw: _dense(capi, **kw)) if call == "dense" else (lambda **kw: _windows(capi, [GOOD], **kw))
    for G in (0, -1, 257, 1 << 20):
        assert f(G=G, max_score=[1.0] * 300, min_matched=None) == EINVAL and "n_objects must be in [1, 256]" in _err(capi)
    assert f(max_score=None) == EINVAL and "max_score is null" in _err(capi)
    for bad in (np.nan, -1.0, -INF):
        assert f(max_score=(1.0, bad)) == EINVAL and "max_score must be >= 0" in _err(capi)
    for bad in (np.nan, -0.5, 1.5, float(np.nextafter(np.float32(1), np.float32(2)))):
        assert f(min_matched=(0.5, bad)) == EINVAL and "min_matched must be in [0, 1]" in _err(capi)
    for cross in (-1, 1001):
        assert f(cross=cross) == EINVAL and "cross_permille must be in [0, 1000]" in _err(capi)
    for gate in (-1, 2, 1 << 30):
        assert f(gate=gate) == EINVAL and "gate must be FDCM_GATE_WINNER or FDCM_GATE_ALL" in _err(capi)


@pytest.mark.parametrize("gate", [0, 1])
def test_what_the_dense_sibling_rejects(capi, gate):
    d = lambda **kw: _dense(capi, gate=gate, **kw)
    for md in (0, 4097, -1):
        assert d(max_det=md) == EINVAL and "max_detections must be in [1, 4096]" in _err(capi)
    for permille in (-1, 1001):
        assert d(permille=permille) == EINVAL and "overlap_permille must be in [0, 1000]" in _err(capi)
    for margin in (-1, 4097):
        assert d(margin=margin) == EINVAL and "margin must be in [0, 4096]" in _err(capi)
    assert d(out=False) == EINVAL and "null output" in _err(capi)
    assert d(n_out=False) == EINVAL and "null output" in _err(capi)
    assert d(grid=None) == EINVAL and "grid is null" in _err(capi)
    for grid, what in [((0, 0, 4, 4, 0, 1), "stride"), ((0, 0, 0, 4, 1, 1), "nx and ny"), ((0, 0, (1 << 13) + 1, 1 << 13, 1, 1), "2^26"),
                       ((0, 0, (1 << 13) + 1, 1 << 12, 1, 1), "n_objects * nx * ny must be at most 2^26")]:
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
    for G in (0, 257):
        assert _map(capi, G=G, min_matched=None) == EINVAL and "n_objects must be in [1, 256]" in _err(capi)
    for bad in (np.nan, -0.5, 1.5):
        assert _map(capi, min_matched=(bad, 0.0)) == EINVAL and "min_matched must be in [0, 1]" in _err(capi)
    assert _map(capi, grid=None) == EINVAL and "grid is null" in _err(capi)
    for grid, what in [((0, 0, 4, 4, 1, 0), "stride"), ((0, 0, 4, 0, 1, 1), "nx and ny"),
                       ((0, 0, (1 << 13) + 1, 1 << 12, 1, 1), "n_objects * nx * ny must be at most 2^26")]:
        assert _map(capi, grid=grid) == EINVAL and what in _err(capi)
    assert _map(capi, penalty=3) == EINVAL and "unknown penalty" in _err(capi)
    assert _map(capi, penalty=1, tau=np.nan) == EINVAL and "tau must be finite" in _err(capi)
    assert _map(capi, rot=capi.Rotations(None, 3, None)) == EINVAL and "cs is null" in _err(capi)


@pytest.mark.parametrize("gate", [0, 1])
def test_what_the_windows_sibling_rejects(capi, gate):
    w = lambda jobs=(GOOD,), **kw: _windows(capi, list(jobs) if jobs is not None else None, gate=gate, **kw)
    for kw, what in [
        (dict(max_det=0), "max_detections must be in [1, 4096]"), (dict(max_det=4097), "max_detections must be in [1, 4096]"),
        (dict(permille=-1), "overlap_permille must be in [0, 1000]"), (dict(permille=1001), "overlap_permille must be in [0, 1000]"),
        (dict(margin=-1), "margin must be in [0, 4096]"), (dict(margin=4097), "margin must be in [0, 4096]"),
        (dict(penalty=2), "unknown penalty"), (dict(tau=float("inf")), "tau must be finite"),
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
    bad = np.float32([[1, 0], [np.nan, 0]])
    assert w(rot=capi.Rotations(capi.fptr(bad), 2, None)) == EINVAL and "c and s must be finite" in _err(capi)
    assert w(rot=capi.Rotations(None, 2, None)) == EINVAL and "cs is null" in _err(capi)


def test_python_signatures(capi):
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap, object_arrays
    p = inspect.signature(fd.object_score_maps).parameters
    assert list(p) == ["featuremap", "templates", "objects", "stride", "penalty", "angles", "pivot", "window", "line_caps", "min_matched",
                       "return_matched", "n_objects"]
    assert p["stride"].default == 1 and p["pivot"].default == "center" and p["min_matched"].default is None
    assert p["return_matched"].default is False and p["n_objects"].default is None
    p = inspect.signature(fd.exhaustive_detect_objects).parameters
    assert list(p)[:6] == ["featuremap", "templates", "objects", "max_score", "overlap", "cross_overlap"] and list(p)[-1] == "gate"
    assert p["overlap"].default == 0.3 and p["cross_overlap"].default is None and p["n_objects"].default is None
    assert p["return_objects"].default is False and p["gate"].default == "winner" and p["max_detections"].default == 1024
    # the remaining keywords are exhaustive_detect_all's, with its defaults
    old = inspect.signature(fd.exhaustive_detect_all).parameters
    for name in list(old)[3:]:
        assert name in p and p[name].default == old[name].default, name
    p = inspect.signature(fd.exhaustive_detect_windows_objects).parameters
    assert list(p)[:7] == ["featuremap", "templates", "jobs", "objects", "max_score", "overlap", "cross_overlap"] and list(p)[-1] == "gate"
    old = inspect.signature(fd.exhaustive_detect_windows).parameters
    for name in list(old)[4:]:
        assert name in p and p[name].default == old[name].default, name
    assert p["return_objects"].default is False and p["cross_overlap"].default is None
    p = inspect.signature(fd.exhaustive_detect_refined_objects).parameters
    assert list(p)[:10] == ["featuremap", "templates", "objects", "max_score", "coarse_angles", "fine_angles", "coarse_stride", "half_angles",
                            "half_x", "half_y"]
    old = inspect.signature(fd.exhaustive_detect_refined).parameters
    for name in list(old)[9:]:
        assert name in p and p[name].default == old[name].default, name
    doc = fd.exhaustive_detect_refined_objects.__doc__
    assert "exhaustive_detect_objects(" in doc and "pose_windows(" in doc and "exhaustive_detect_windows_objects(" in doc
    for name in ("best_map_objects", "exhaustive_detect_objects", "exhaustive_detect_windows_objects"):
        q = inspect.signature(getattr(DeviceFeatureMap, name)).parameters
        assert "objects" in q and q["n_objects"].default is None and q["cs"].default is None
    # the functions that were there keep their parameters
    p = inspect.signature(fd.exhaustive_detect_all).parameters
    assert list(p) == ["featuremap", "templates", "max_score", "overlap", "stride", "max_detections", "penalty", "angles", "pivot", "window",
                       "line_caps", "margin", "return_boxes", "min_matched", "return_matched", "gate"]
    p = inspect.signature(fd.best_score_map).parameters
    assert list(p) == ["featuremap", "templates", "stride", "penalty", "angles", "pivot", "window", "line_caps", "min_matched",
                       "return_matched"]
    assert list(inspect.signature(fd.exhaustive_detect_windows).parameters)[-4:] == ["return_boxes", "return_matched", "return_jobs", "gate"]
    assert list(inspect.signature(fd.exhaustive_detect_refined).parameters)[-1] == "gate"
    assert list(inspect.signature(DeviceFeatureMap.best_map).parameters) == ["self", "templates", "grid", "cs", "pivots", "penalty", "tau",
                                                                             "min_matched", "matched"]
    # the per-object arguments: a scalar for all, or one value per object
    obj, G, ms, mm = object_arrays([2, 0, 2], None, 3, 1.5, None)
    assert obj.dtype == np.int32 and G == 3 and ms.tolist() == [1.5] * 3 and mm is None
    obj, G, ms, mm = object_arrays([0, 0], 4, 2, [1, 2, 3, INF], 0.25)
    assert G == 4 and ms.dtype == np.float32 and ms[3] == INF and mm.tolist() == [0.25] * 4
    for bad in (lambda: object_arrays([0, 1], None, 3, 1.0, None), lambda: object_arrays([0, 1], None, 2, [1.0], None),
                lambda: object_arrays([0.5, 1], None, 2, 1.0, None)):
        with pytest.raises(ValueError):
            bad()
    for call in (fd.exhaustive_detect_objects, fd.exhaustive_detect_refined_objects):
        with pytest.raises(ValueError, match="gate must be"):
            call(None, None, None, *([None] * (8 if call is fd.exhaustive_detect_refined_objects else 1)), gate="best")
    with pytest.raises(ValueError, match="gate must be"):
        fd.exhaustive_detect_windows_objects(None, None, None, None, None, gate="best")
