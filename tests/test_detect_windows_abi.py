"""CPU-only checks of the detections over pose windows (include/fdcm.h, "Detections over pose windows"): the library exports
the entry point, the binding knows its prototype, and every argument check of the header's list returns FDCM_EINVAL with a
message before any handle or device is touched (the handles are null here: a check that came late would report "null
featuremap/templates").  A template index past the end of a set and the empty inputs (no jobs, an empty map, an empty set:
FDCM_OK and zero records) need handles, which need a device: test_gpu_detect_windows.py has those."""
import ctypes as C
import os

import numpy as np
import pytest

EINVAL = -1
INF = float("inf")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def _rot(capi, n):
    cs = np.tile(np.float32([[1, 0]]), (n, 1))
    return capi.Rotations(capi.fptr(cs), n, None), cs


def _call(capi, jobs, rot=None, sx=1, sy=1, wrap=0, max_score=INF, max_detections=100, overlap_permille=300, margin=0, penalty=0,
          tau=1.0, min_matched=0.0, n_jobs=None, out=True, n_out=True):
    jobs = None if jobs is None else np.ascontiguousarray(np.asarray(jobs, dtype=np.int32).reshape(-1, 7))
    o, n = C.c_void_p(), C.c_int64()
    return capi.lib().fdcm_search_exhaustive_detect_windows(
        None, None, C.byref(rot) if rot is not None else None,
        jobs.ctypes.data_as(C.POINTER(capi.PoseWindow)) if jobs is not None else None,
        (0 if jobs is None else jobs.shape[0]) if n_jobs is None else n_jobs, sx, sy, wrap, max_score, max_detections, overlap_permille,
        margin, penalty, tau, min_matched, 0, C.byref(o) if out else None, C.byref(n) if n_out else None, None, None, None)


GOOD = (0, 0, 1, -4, -4, 9, 9)


def test_exports_binds_and_declares(capi):
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "fdcm_search_exhaustive_detect_windows")
    proto = {s[0]: s for s in capi.SYMBOLS}["fdcm_search_exhaustive_detect_windows"]
    assert proto[1] is C.c_int and len(proto[2]) == 21
    assert proto[2][3] == C.POINTER(capi.PoseWindow) and proto[2][4] is C.c_int64 and proto[2][8] is C.c_float
    assert proto[2][13] is C.c_float and proto[2][14] is C.c_float and proto[2][19] == C.POINTER(C.c_float)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(capi.LIB_PATH)), "include", "fdcm.h")).read()
    assert "int fdcm_search_exhaustive_detect_windows(" in hdr and "Detections over pose windows" in hdr
    import openfdcm_amd
    from openfdcm_amd.engine import DeviceFeatureMap
    assert callable(DeviceFeatureMap.exhaustive_detect_windows)
    assert callable(openfdcm_amd.exhaustive_detect_windows) and callable(openfdcm_amd.exhaustive_detect_refined)


def test_valid_arguments_reach_the_null_handles(capi):
    """The reference point of the tests below: good arguments fail only at the handles."""
    rot, keep = _rot(capi, 4)
    assert _call(capi, [GOOD]) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _call(capi, [(3, 3, 2, -4, -4, 9, 9)], rot=rot, wrap=1, max_score=0.0, max_detections=4096, overlap_permille=1000, margin=4096,
                 penalty=-1, min_matched=1.0) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _call(capi, [GOOD], max_detections=1, overlap_permille=0, penalty=1, tau=1.5) == EINVAL and "null featuremap" in _err(capi)
    assert _call(capi, None, n_jobs=0) == EINVAL and "null featuremap/templates" in _err(capi)


@pytest.mark.parametrize("kw,what", [
    (dict(max_score=float("nan")), "max_score must be >= 0"), (dict(max_score=-1.0), "max_score must be >= 0"),
    (dict(max_detections=0), "max_detections must be in [1, 4096]"), (dict(max_detections=4097), "max_detections must be in [1, 4096]"),
    (dict(overlap_permille=-1), "overlap_permille must be in [0, 1000]"), (dict(overlap_permille=1001), "overlap_permille must be in [0, 1000]"),
    (dict(margin=-1), "margin must be in [0, 4096]"), (dict(margin=4097), "margin must be in [0, 4096]"),
    (dict(penalty=2), "unknown penalty"), (dict(penalty=-2), "unknown penalty"),
    (dict(tau=float("inf")), "tau must be finite"), (dict(tau=float("nan")), "tau must be finite"),
    (dict(min_matched=float("nan")), "min_matched must be in [0, 1]"), (dict(min_matched=-0.5), "min_matched must be in [0, 1]"),
    (dict(min_matched=1.5), "min_matched must be in [0, 1]"),
])
def test_what_the_detector_rejects(capi, kw, what):
    assert _call(capi, [GOOD], **kw) == EINVAL and what in _err(capi)


def test_job_list_pointer_and_count(capi):
    assert _call(capi, None, n_jobs=1) == EINVAL and "jobs is null" in _err(capi)
    assert _call(capi, [GOOD], n_jobs=-1) == EINVAL and "n_jobs is negative" in _err(capi)
    assert _call(capi, [GOOD], n_jobs=(1 << 22) + 1) == EINVAL and "n_jobs must be at most 2^22" in _err(capi)  # before any job is read
    many = np.tile(np.int32([GOOD]), (1 << 22, 1))
    assert _call(capi, many) == EINVAL and "null featuremap/templates" in _err(capi)  # the limit itself


@pytest.mark.parametrize("sx,sy", [(0, 1), (1, 0), (-2, 1)])
def test_strides_below_one(capi, sx, sy):
    assert _call(capi, [GOOD], sx=sx, sy=sy) == EINVAL and "strides sx and sy must be >= 1" in _err(capi)


@pytest.mark.parametrize("wrap", [-1, 2])
def test_wrap_not_boolean(capi, wrap):
    assert _call(capi, [GOOD], wrap=wrap) == EINVAL and "wrap must be 0 or 1" in _err(capi)


@pytest.mark.parametrize("job,n,wrap,what", [
    ((-1, 0, 1, 0, 0, 3, 3), 4, 0, "tmpl is outside the template set"),
    ((0, 0, 0, 0, 0, 3, 3), 4, 0, "na must be in [1, n]"),
    ((0, 0, 5, 0, 0, 3, 3), 4, 1, "na must be in [1, n]"),
    ((0, -1, 1, 0, 0, 3, 3), 4, 1, "a0 must be in [0, n - 1]"),
    ((0, 4, 1, 0, 0, 3, 3), 4, 1, "a0 must be in [0, n - 1]"),
    ((0, 3, 2, 0, 0, 3, 3), 4, 0, "a0 + na must be at most n without wrap"),
    ((0, 0, 1, 0, 0, 0, 3), 4, 0, "nx and ny must be >= 1"),
    ((0, 0, 1, 0, 0, 3, -1), 4, 0, "nx and ny must be >= 1"),
    ((0, 0, 1, 0, 0, 257, 256), 4, 0, "na * nx * ny must be at most 65536"),
    ((0, 0, 2, 0, 0, 256, 129), 4, 0, "na * nx * ny must be at most 65536"),
    ((0, 0, 1, -(1 << 24), 0, 3, 3), 4, 0, "|t| < 2^24"),
    ((0, 0, 1, 0, (1 << 24) - 2, 3, 3), 4, 0, "|t| < 2^24"),
])
def test_job_limits(capi, job, n, wrap, what):
    """One bad job behind a good one: every job is checked."""
    rot, keep = _rot(capi, n)
    assert _call(capi, [(0, 0, 1, 0, 0, 3, 3), job], rot=rot, wrap=wrap) == EINVAL
    assert what in _err(capi)


def test_translations_only_and_what_the_rotation_call_rejects_about_rot(capi):
    assert _call(capi, [(0, 1, 1, 0, 0, 3, 3)]) == EINVAL and "a0 must be in [0, n - 1]" in _err(capi)
    assert _call(capi, [(0, 0, 2, 0, 0, 3, 3)], wrap=1) == EINVAL and "na must be in [1, n]" in _err(capi)
    cs = np.float32([[1, 0], [np.nan, 0]])
    assert _call(capi, [GOOD], rot=capi.Rotations(capi.fptr(cs), 2, None)) == EINVAL and "c and s must be finite" in _err(capi)
    assert _call(capi, [GOOD], rot=capi.Rotations(capi.fptr(cs), 0, None)) == EINVAL and "n must be >= 1" in _err(capi)
    assert _call(capi, [GOOD], rot=capi.Rotations(None, 2, None)) == EINVAL and "cs is null" in _err(capi)


def test_null_outputs(capi):
    assert _call(capi, [GOOD], out=False) == EINVAL and "null output" in _err(capi)
    assert _call(capi, [GOOD], n_out=False) == EINVAL and "null output" in _err(capi)
