"""CPU-only checks of the pose-window search (include/fdcm.h, "Pose windows"): the library exports the entry point, the
binding knows it and the struct's layout, and every argument check of the header's list returns FDCM_EINVAL with a message
before any handle or device is touched (the handles are null here: a check that came late would report "null").  A template
index past the end of a set needs a set, which needs a device: test_gpu_exhaustive_windows.py has that one."""
import ctypes as C
import os

import numpy as np
import pytest

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


def _rot(capi, n):
    cs = np.tile(np.float32([[1, 0]]), (n, 1))
    return capi.Rotations(capi.fptr(cs), n, None), cs


def _call(capi, jobs, rot=None, sx=1, sy=1, wrap=0, k=1, n_jobs=None, out=True, offsets=None):
    jobs = None if jobs is None else np.ascontiguousarray(np.asarray(jobs, dtype=np.int32).reshape(-1, 7))
    o, n = C.c_void_p(), C.c_int64()
    return capi.lib().fdcm_search_exhaustive_windows(
        None, None, C.byref(rot) if rot is not None else None,
        jobs.ctypes.data_as(C.POINTER(capi.PoseWindow)) if jobs is not None else None,
        (0 if jobs is None else jobs.shape[0]) if n_jobs is None else n_jobs, sx, sy, wrap, k, 0,
        C.byref(o) if out else None, C.byref(n) if out else None, offsets)


GOOD = (0, 0, 1, -4, -4, 9, 9)


def test_exports_binds_and_lays_out_the_struct(capi):
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "fdcm_search_exhaustive_windows")
    assert "fdcm_search_exhaustive_windows" in {s[0] for s in capi.SYMBOLS}
    assert C.sizeof(capi.PoseWindow) == 28 and capi.POSE_WINDOW_DTYPE.itemsize == 28
    names = ["tmpl", "a0", "na", "x0", "y0", "nx", "ny"]
    assert [f[0] for f in capi.PoseWindow._fields_] == names and list(capi.POSE_WINDOW_DTYPE.names) == names
    for i, nm in enumerate(names):
        assert getattr(capi.PoseWindow, nm).offset == 4 * i and getattr(capi.PoseWindow, nm).size == 4
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(capi.LIB_PATH)), "include", "fdcm.h")).read()
    assert "typedef struct fdcm_pose_window" in hdr and "int fdcm_search_exhaustive_windows(" in hdr
    import openfdcm_amd
    from openfdcm_amd.engine import DeviceFeatureMap, as_pose_windows
    assert callable(DeviceFeatureMap.exhaustive_window_search) and callable(openfdcm_amd.exhaustive_window_search)
    assert callable(openfdcm_amd.pose_windows)
    rows = as_pose_windows(np.array([GOOD], dtype=capi.POSE_WINDOW_DTYPE))
    assert rows.dtype == np.int32 and rows.tolist() == [list(GOOD)]
    with pytest.raises(ValueError):
        as_pose_windows(np.zeros((2, 6), dtype=np.int32))


def test_a_valid_job_list_reaches_the_null_handles(capi):
    """The reference point of the tests below: good arguments fail only at the handles."""
    rot, keep = _rot(capi, 4)
    assert _call(capi, [GOOD]) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _call(capi, [(3, 2, 2, -4, -4, 9, 9)], rot=rot) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _call(capi, [(3, 3, 2, -4, -4, 9, 9)], rot=rot, wrap=1) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _call(capi, None, n_jobs=0) == EINVAL and "null featuremap/templates" in _err(capi)


def test_job_list_pointer_and_count(capi):
    assert _call(capi, None, n_jobs=1) == EINVAL and "jobs is null" in _err(capi)
    assert _call(capi, [GOOD], n_jobs=-1) == EINVAL and "n_jobs is negative" in _err(capi)


@pytest.mark.parametrize("k", [0, 65, -1])
def test_k_out_of_range(capi, k):
    assert _call(capi, [GOOD], k=k) == EINVAL and "k must be in [1, 64]" in _err(capi)


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
    ((0, 0, 1, 0, 0, 1 << 30, 1 << 30), 4, 0, "na * nx * ny must be at most 65536"),
    ((0, 0, 1, -(1 << 24), 0, 3, 3), 4, 0, "|t| < 2^24"),
    ((0, 0, 1, 0, (1 << 24) - 2, 3, 3), 4, 0, "|t| < 2^24"),
])
def test_job_limits(capi, job, n, wrap, what):
    """One bad job behind a good one: every job is checked."""
    rot, keep = _rot(capi, n)
    assert _call(capi, [(0, 0, 1, 0, 0, 3, 3), job], rot=rot, wrap=wrap) == EINVAL
    assert what in _err(capi)


def test_the_limit_itself_and_the_stride_in_the_range_check(capi):
    rot, keep = _rot(capi, 4)
    for job in [(0, 0, 1, 0, 0, 256, 256), (0, 0, 4, 0, 0, 128, 128), (0, 0, 1, (1 << 24) - 3, -(1 << 24) + 1, 3, 3)]:
        assert _call(capi, [job], rot=rot) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _call(capi, [(0, 0, 1, (1 << 24) - 5, 0, 3, 3)], rot=rot, sx=2) == EINVAL and "null featuremap" in _err(capi)
    assert _call(capi, [(0, 0, 1, (1 << 24) - 5, 0, 3, 3)], rot=rot, sx=3) == EINVAL and "|t| < 2^24" in _err(capi)


def test_translations_only_is_a_table_of_one_rotation(capi):
    """rot == NULL: a0 = 0 and na = 1 are the only run."""
    assert _call(capi, [(0, 1, 1, 0, 0, 3, 3)]) == EINVAL and "a0 must be in [0, n - 1]" in _err(capi)
    assert _call(capi, [(0, 0, 2, 0, 0, 3, 3)]) == EINVAL and "na must be in [1, n]" in _err(capi)
    assert _call(capi, [(0, 0, 2, 0, 0, 3, 3)], wrap=1) == EINVAL and "na must be in [1, n]" in _err(capi)


def test_what_the_rotation_call_rejects_about_rot(capi):
    cs = np.float32([[1, 0], [np.nan, 0]])
    bad = capi.Rotations(capi.fptr(cs), 2, None)
    assert _call(capi, [GOOD], rot=bad) == EINVAL and "c and s must be finite" in _err(capi)
    bad = capi.Rotations(capi.fptr(cs), 0, None)
    assert _call(capi, [GOOD], rot=bad) == EINVAL and "n must be >= 1" in _err(capi)
    bad = capi.Rotations(None, 2, None)
    assert _call(capi, [GOOD], rot=bad) == EINVAL and "cs is null" in _err(capi)


def test_null_outputs(capi):
    assert _call(capi, [GOOD], out=False) == EINVAL and "null" in _err(capi)
