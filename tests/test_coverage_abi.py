"""Checks of scene coverage (include/fdcm.h, "Scene coverage") that need no scene: the library exports the entry point, the
binding and the header know it, the Python names have the stated signatures, and every argument check that can be reached
without a handle returns FDCM_EINVAL with its own message before any handle or device is touched (the handles are NULL
throughout: a late check would report them instead).  record_poses is pure numpy and is held to its definition here."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

EINVAL = -1
LAB = np.zeros(4096 * 4096, dtype=np.uint8)   # the largest image the call takes (never read here): the overlap check looks at the full extents
RES = np.zeros(4096 * 4096, dtype=np.uint8)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def _cov(capi, poses=((0, 0, 0, 0),), rot=None, n=None, params=(2, 1, 2), labels=True, width=16, height=12, counts=True, residual=False,
         overlap=False):
    p = np.ascontiguousarray(poses, dtype=np.int32).reshape(-1, 4)
    lab, res = LAB, RES
    out = np.zeros((max(1, len(p)), 2), dtype=np.int32)
    par = capi.CoverageParams(*params) if params is not None else None
    rp = C.c_void_p(lab.ctypes.data + 5) if overlap else C.c_void_p(res.ctypes.data)
    return capi.lib().fdcm_scene_coverage(None, C.c_void_p(lab.ctypes.data) if labels else None, width, height, 0, None,
                                          C.byref(rot) if rot is not None else None,
                                          p.ctypes.data_as(C.POINTER(C.c_int32)) if len(p) else None, len(p) if n is None else n,
                                          C.byref(par) if par is not None else None,
                                          out.ctypes.data_as(C.POINTER(C.c_int32)) if counts else None, rp if residual or overlap else None)


def test_exports_declares_and_binds_the_entry_point(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    assert hasattr(lib, "fdcm_scene_coverage") and "fdcm_scene_coverage" in bound
    assert len(bound["fdcm_scene_coverage"][2]) == 12 and bound["fdcm_scene_coverage"][1] is C.c_int
    assert C.sizeof(capi.CoverageParams) == 12
    assert [(n, t) for n, t in capi.CoverageParams._fields_] == [("radius", C.c_int32), ("bin_tolerance", C.c_int32), ("margin", C.c_int32)]
    with open(os.path.join(os.path.dirname(capi.LIB_PATH), "..", "include", "fdcm.h")) as f:
        header = f.read()
    decl = re.search(r"int fdcm_scene_coverage\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S)
    assert decl and len(decl.group(1).split(",")) == 12
    assert "typedef struct fdcm_coverage_params {" in header and "} fdcm_coverage_params;" in header
    assert "Scene coverage" in header and "tests/coverage_ref.py" in header
    root = os.path.join(os.path.dirname(capi.LIB_PATH), "..")
    with open(os.path.join(root, "openfdcm_amd", "csrc", "Makefile")) as f:
        assert "fdcm_coverage.hip" in f.read()
    with open(os.path.join(root, "openfdcm_amd", "csrc", "fdcm_internal.h")) as f:
        assert "run_scene_coverage" in f.read()
    with open(os.path.join(root, "README.md")) as f:
        assert "Scene coverage" in f.read()


def test_python_signatures(capi):
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap
    p = inspect.signature(fd.scene_coverage).parameters
    assert list(p) == ["featuremap", "labels", "templates", "poses", "angles", "pivot", "radius", "bin_tolerance", "margin", "return_residual"]
    assert p["angles"].default is None and p["pivot"].default == "center" and p["radius"].default == 2 and p["bin_tolerance"].default == 1
    assert p["margin"].default is None and p["return_residual"].default is False
    p = inspect.signature(fd.record_poses).parameters
    assert list(p) == ["records", "angles", "pivots"] and p["angles"].default is None and p["pivots"].default is None
    p = inspect.signature(DeviceFeatureMap.scene_coverage).parameters
    assert list(p) == ["self", "labels", "templates", "poses", "cs", "pivots", "radius", "bin_tolerance", "margin", "residual"]
    assert p["cs"].default is None and p["pivots"].default is None and p["radius"].default == 2 and p["bin_tolerance"].default == 1
    assert p["margin"].default is None and p["residual"].default is False


def test_no_existing_public_signature_changed(capi):
    """The change is additive: the parameter lists the existing tests state are the ones found."""
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap
    assert list(inspect.signature(fd.exhaustive_detect_all).parameters) == [
        "featuremap", "templates", "max_score", "overlap", "stride", "max_detections", "penalty", "angles", "pivot", "window", "line_caps",
        "margin", "return_boxes", "min_matched", "return_matched", "gate"]
    assert list(inspect.signature(fd.matched_fractions).parameters) == ["featuremap", "templates", "poses", "angles", "pivot", "line_caps"]
    assert list(inspect.signature(fd.line_costs).parameters) == ["featuremap", "templates", "poses", "angles", "pivot"]
    assert list(inspect.signature(fd.pose_windows).parameters) == ["records", "coarse_angles", "fine_angles", "pivots", "half_angles", "half_x",
                                                                    "half_y", "stride", "wrap"]
    assert list(inspect.signature(DeviceFeatureMap.matched_fractions).parameters) == ["self", "templates", "poses", "cs", "pivots"]
    assert list(inspect.signature(DeviceFeatureMap.rebuild_labels).parameters) == ["self", "labels", "border"]
    bound = {s[0]: s for s in capi.SYMBOLS}
    assert len(bound["fdcm_line_costs"][2]) == 7 and len(bound["fdcm_matched_fractions"][2]) == 6
    assert len(bound["fdcm_templates_footprints"][2]) == 4 and len(bound["fdcm_featuremap_rebuild_labels"][2]) == 6


def test_valid_arguments_reach_the_handles(capi):
    """The bounds are inclusive: with them the call goes on to the (null) handles."""
    lim = (1 << 24) - 1
    for params in [(0, 0, 0), (32, 0, 4096), (2, 1 << 20, 2)]:       # bin_tolerance's upper bound needs the map
        for w, h in [(1, 1), (4096, 4096), (1, 4096)]:
            assert _cov(capi, [[0, 0, lim, -lim], [7, 0, 0, 0]], params=params, width=w, height=h, residual=True) == EINVAL
            assert "null featuremap/templates" in _err(capi)
    assert _cov(capi, np.zeros((0, 4)), counts=False) == EINVAL and "null featuremap/templates" in _err(capi)   # n = 0: no arrays
    cs = np.float32([[1, 0], [0, 1]])
    assert _cov(capi, [[0, 1, 3, 4]], rot=capi.Rotations(capi.fptr(cs), 2, None)) == EINVAL and "null featuremap/templates" in _err(capi)


def test_what_the_pose_calls_reject_is_einval(capi):
    assert _cov(capi, n=-1) == EINVAL and "n is negative" in _err(capi)
    assert _cov(capi, np.zeros((0, 4)), n=2) == EINVAL and "poses is null" in _err(capi)
    assert _cov(capi, [[-1, 0, 0, 0]]) == EINVAL and "tmpl is outside the template set" in _err(capi)
    assert _cov(capi, [[0, 1, 0, 0]]) == EINVAL and "a must be 0 without rotations" in _err(capi)
    assert _cov(capi, [[0, -1, 0, 0]]) == EINVAL and "a must be 0 without rotations" in _err(capi)
    cs = np.float32([[1, 0], [0, 1]])
    rot = capi.Rotations(capi.fptr(cs), 2, None)
    assert _cov(capi, [[0, 2, 0, 0]], rot=rot) == EINVAL and "a must be in [0, n - 1]" in _err(capi)
    for x, y in [(1 << 24, 0), (0, -(1 << 24))]:
        assert _cov(capi, [[0, 0, x, y]]) == EINVAL and "|t| < 2^24" in _err(capi)
    bad = np.float32([[1, 0], [np.inf, 0]])
    assert _cov(capi, rot=capi.Rotations(capi.fptr(bad), 2, None)) == EINVAL and "c and s must be finite" in _err(capi)
    assert _cov(capi, rot=capi.Rotations(None, 3, None)) == EINVAL and "cs is null" in _err(capi)


def test_what_the_call_itself_rejects_is_einval(capi):
    many = np.zeros(((1 << 20) + 1, 4), dtype=np.int32)
    assert _cov(capi, many) == EINVAL and "n must be at most 2^20" in _err(capi)
    assert _cov(capi, many[:-1]) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _cov(capi, params=None) == EINVAL and "params is null" in _err(capi)
    for r in (-1, 33):
        assert _cov(capi, params=(r, 1, 2)) == EINVAL and "radius must be in [0, 32]" in _err(capi)
    assert _cov(capi, params=(2, -1, 2)) == EINVAL and "bin_tolerance must be in [0, m / 2]" in _err(capi)
    for mg in (-1, 4097):
        assert _cov(capi, params=(2, 1, mg)) == EINVAL and "margin must be in [0, 4096]" in _err(capi)
    assert _cov(capi, labels=False) == EINVAL and "labels is null" in _err(capi)
    for w, h in [(0, 12), (16, 0), (4097, 12), (16, 4097), (-1, 12)]:
        assert _cov(capi, width=w, height=h) == EINVAL and "width and height must be in [1, 4096]" in _err(capi)
    assert _cov(capi, counts=False) == EINVAL and "counts_out is null" in _err(capi)
    assert _cov(capi, overlap=True) == EINVAL and "residual_out must not overlap labels" in _err(capi)
    # in the order of the section: the pose list before the parameters, the parameters before the image
    assert _cov(capi, n=-1, params=None, labels=False) == EINVAL and "n is negative" in _err(capi)
    assert _cov(capi, params=None, labels=False) == EINVAL and "params is null" in _err(capi)
    assert _cov(capi, params=(2, 1, 9999), labels=False, width=0) == EINVAL and "margin" in _err(capi)
    assert _cov(capi, labels=False, width=0, counts=False) == EINVAL and "labels is null" in _err(capi)


def _records(tmpl, transforms):
    from openfdcm_amd import _capi
    rec = np.zeros(len(tmpl), dtype=_capi.MATCH_DTYPE)
    rec["tmpl_idx"] = tmpl
    rec["transform"] = np.asarray(transforms, dtype=np.float32)
    return rec


def test_record_poses_is_the_pose_windows_expression():
    import openfdcm_amd as fd
    from rotation_ref import rot_matrix
    rng = np.random.default_rng(11)
    angles = np.linspace(0, 2 * np.pi, 7, endpoint=False)
    cs = np.stack([np.cos(angles), np.sin(angles)], axis=1).astype(np.float32)
    pivots = rng.uniform(-40, 40, size=(5, 2)).astype(np.float32)
    for pv in (pivots, None):
        tmpl = rng.integers(0, 5, size=40)
        a = rng.integers(0, 7, size=40)
        t = rng.integers(-3000, 3000, size=(40, 2))
        tr = []
        for q in range(40):
            M = rot_matrix(cs[a[q], 0], cs[a[q], 1], *((0.0, 0.0) if pv is None else pv[tmpl[q]]))
            tr.append([M[0, 0], M[0, 1], M[0, 2] + np.float32(t[q, 0]), M[1, 0], M[1, 1], M[1, 2] + np.float32(t[q, 1])])
        rec = _records(tmpl, tr)
        got = fd.record_poses(rec, angles, pv)
        want = fd.pose_windows(rec, angles, angles, pv, 0, 0, 0)[:, [0, 1, 3, 4]]
        assert got.dtype == np.int32 and got.shape == (40, 4) and np.array_equal(got, want)
        assert np.array_equal(got, np.stack([tmpl, a, t[:, 0], t[:, 1]], axis=1))
        assert np.array_equal(fd.record_poses(fd.MatchList(rec), angles, pv), want)
    # without angles: the pure translations of the dense calls
    tmpl = rng.integers(0, 5, size=30)
    t = rng.integers(-5000, 5000, size=(30, 2))
    rec = _records(tmpl, [[1, 0, x, 0, 1, y] for x, y in t])
    got = fd.record_poses(rec)
    assert got.dtype == np.int32 and np.array_equal(got, np.stack([tmpl, np.zeros(30, int), t[:, 0], t[:, 1]], axis=1))
    assert fd.record_poses(rec[:0]).shape == (0, 4) and fd.record_poses(rec[:0], angles).shape == (0, 4)
