"""CPU-only checks of the per-line caps and line costs (include/fdcm.h, "Per-line caps and line costs"): the library exports
the entry points and the binding knows them, and every argument check returns FDCM_EINVAL with a message before any handle
or device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

EINVAL = -1
NEW_SYMBOLS = ["fdcm_templates_create_capped", "fdcm_templates_line_caps", "fdcm_templates_line_lengths", "fdcm_line_costs"]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def _costs(capi, poses, rot=None, n=None, outs=True):
    p = np.ascontiguousarray(poses if poses is not None else [], dtype=np.int32).reshape(-1, 4)
    out, off = C.POINTER(C.c_float)(), np.zeros(len(p) + 2, dtype=np.int64)
    return capi.lib().fdcm_line_costs(None, None, C.byref(rot) if rot is not None else None,
                                      p.ctypes.data_as(C.POINTER(C.c_int32)) if poses is not None else None,
                                      len(p) if n is None else n, C.byref(out) if outs else None,
                                      off.ctypes.data_as(C.POINTER(C.c_int64)) if outs else None)


def _rot(capi, cs):
    cs = np.ascontiguousarray(cs, dtype=np.float32).reshape(-1, 2)
    return capi.Rotations(capi.fptr(cs), cs.shape[0], None), cs


def test_exports_and_binds_the_entry_points(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0] for s in capi.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in bound
    import inspect
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    for f in (DeviceFeatureMap.line_costs, DeviceTemplates.line_caps, DeviceTemplates.line_lengths, fd.line_caps, fd.line_costs):
        assert callable(f)
    assert "line_caps" in inspect.signature(DeviceTemplates.__init__).parameters
    for f in (fd.score_map, fd.exhaustive_search, fd.exhaustive_peaks, fd.exhaustive_rotation_search, fd.rotation_score_map,
              fd.exhaustive_window_search, fd.best_score_map, fd.exhaustive_detect):
        assert inspect.signature(f).parameters["line_caps"].default is None
    assert "line_caps" not in inspect.signature(fd.search).parameters
    with open(os.path.join(os.path.dirname(capi.LIB_PATH), "..", "include", "fdcm.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert "int " + name + "(" in header


@pytest.mark.parametrize("bad", [np.nan, -1.0, -np.inf, -1e-30])
def test_bad_caps_are_einval(capi, bad):
    """A NaN or negative cap is rejected before the device is selected, wherever it stands."""
    lines = np.arange(20, dtype=np.float32).reshape(5, 4)
    offsets = np.array([0, 2, 2, 5], dtype=np.int64)
    for at in (0, 3, 4):
        caps = np.float32([0.0, np.inf, 2.5, 1e30, 0.0])
        caps[at] = bad
        h = C.c_void_p(1)
        rc = capi.lib().fdcm_templates_create_capped(capi.fptr(lines), offsets.ctypes.data_as(C.POINTER(C.c_int64)), 3,
                                                     capi.fptr(caps), C.byref(h))
        assert rc == EINVAL and "caps must be >= 0" in _err(capi) and not h.value


def test_create_capped_checks_its_arguments(capi):
    lines = np.zeros((2, 4), dtype=np.float32)
    caps = np.zeros(2, dtype=np.float32)
    off = lambda *v: np.array(v, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    h = C.c_void_p()
    f = capi.lib().fdcm_templates_create_capped
    assert f(capi.fptr(lines), off(0, 2), 1, capi.fptr(caps), None) == EINVAL and "out is null" in _err(capi)
    assert f(capi.fptr(lines), None, 1, capi.fptr(caps), C.byref(h)) == EINVAL and "bad offsets" in _err(capi)
    assert f(capi.fptr(lines), off(0, 2), -1, capi.fptr(caps), C.byref(h)) == EINVAL and "bad offsets" in _err(capi)
    assert f(capi.fptr(lines), off(1, 2), 1, capi.fptr(caps), C.byref(h)) == EINVAL and "offsets[0]" in _err(capi)
    assert f(capi.fptr(lines), off(0, 2, 1), 2, capi.fptr(caps), C.byref(h)) == EINVAL and "ascending" in _err(capi)
    assert capi.lib().fdcm_templates_line_caps(None, capi.fptr(caps)) == EINVAL and "null" in _err(capi)
    assert capi.lib().fdcm_templates_line_lengths(None, capi.fptr(caps)) == EINVAL and "null" in _err(capi)


def test_line_costs_count_and_pointer_checks(capi):
    assert _costs(capi, [[0, 0, 0, 0]], n=-1) == EINVAL and "n is negative" in _err(capi)
    assert _costs(capi, None, n=3) == EINVAL and "poses is null" in _err(capi)
    assert _costs(capi, None, n=0) == EINVAL and "null featuremap/templates" in _err(capi)  # no poses needed: on to the handles
    assert _costs(capi, [[0, 0, 0, 0]]) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _costs(capi, [[0, 0, 0, 0]], outs=False) == EINVAL  # (the handles are checked first)


@pytest.mark.parametrize("pose,what", [
    ((-1, 0, 0, 0), "tmpl is outside"), ((0, 1, 0, 0), "a must be 0"), ((0, -1, 0, 0), "a must be 0"),
    ((0, 0, 1 << 24, 0), "2^24"), ((0, 0, -(1 << 24), 0), "2^24"), ((0, 0, 0, 1 << 24), "2^24"), ((0, 0, 0, -(1 << 24)), "2^24"),
    ((0, 0, 0, -(1 << 31)), "2^24"),
])
def test_bad_poses_are_einval(capi, pose, what):
    """Checked for every pose of the list, before the handles (null here)."""
    good = (0, 0, (1 << 24) - 1, -(1 << 24) + 1)
    assert _costs(capi, [good]) == EINVAL and "null featuremap/templates" in _err(capi)
    for poses in ([pose], [good, good, pose], [pose, good]):
        assert _costs(capi, poses) == EINVAL and what in _err(capi)


def test_angle_index_against_the_rotation_table(capi):
    r, keep = _rot(capi, [[1, 0], [0, 1], [-1, 0]])
    assert _costs(capi, [[0, 2, 5, 5]], rot=r) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _costs(capi, [[0, 3, 5, 5]], rot=r) == EINVAL and "a must be in [0, n - 1]" in _err(capi)
    assert _costs(capi, [[0, -1, 5, 5]], rot=r) == EINVAL and "a must be in [0, n - 1]" in _err(capi)


def test_rotation_checks_are_einval(capi):
    """What the rotation call rejects about a table, when there is one; checked before the handles (null here)."""
    for cs, what in [(np.zeros((0, 2)), "n must be >= 1"), ([[1, 0], [np.nan, 0]], "c and s must be finite"),
                     ([[1, np.inf]], "c and s must be finite")]:
        r, keep = _rot(capi, cs)
        assert _costs(capi, [[0, 0, 0, 0]], rot=r) == EINVAL and what in _err(capi)
    r = capi.Rotations(None, 3, None)
    assert _costs(capi, [[0, 0, 0, 0]], rot=r) == EINVAL and "cs is null" in _err(capi)


def test_python_caps_arguments():
    """The flat caps of a list: a scalar tau is float32(tau) * len_i; arrays are checked for shape and values."""
    import openfdcm_amd as fd
    from openfdcm_amd.engine import flat_line_caps
    tm = [np.float32([[0, 0, 3, 4], [1, 1, 1, 6]]).T.copy(), np.zeros((4, 0), dtype=np.float32), np.float32([[2, 0, 2, 0.5]]).T.copy()]
    per = fd.line_caps(tm, 1.5)
    assert [c.tolist() for c in per] == [[7.5, 7.5], [], [0.75]] and all(c.dtype == np.float32 for c in per)
    assert flat_line_caps(tm, None) is None
    assert flat_line_caps(tm, 1.5).tolist() == [7.5, 7.5, 0.75]
    assert flat_line_caps(tm, [[0, np.inf], [], [2]]).tolist() == [0, np.inf, 2]
    for bad in ([[1, 2], [], []], [[1, 2], [3]], [[1, np.nan], [], [2]], [[1, -2], [], [2]]):
        with pytest.raises(ValueError):
            flat_line_caps(tm, bad)
