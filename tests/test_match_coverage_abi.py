"""Checks of scene coverage and selection of match records (include/fdcm.h, "Match lists: scene coverage and selection") that
need no scene: the library exports the entry points, the binding and the header know them, the Python names have the stated
signatures and defaults, a MatchList indexed by a selection is a MatchList, and every argument check returns FDCM_EINVAL with
its own message before any handle or device is touched (the handles are NULL throughout: a late check would report them
instead)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

EINVAL = -1
LAB = np.zeros(4096 * 4096, dtype=np.uint8)   # the largest image the calls take (never read here)
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


def _call(capi, select, n=1, matches=True, on_device=0, params=(2, 1, 2), sel=(0, 500, 1, 1024), labels=True, width=16, height=12,
          selected=True, counts=True, n_out=True, residual=False, overlap=False):
    rec = np.zeros(1, dtype=capi.MATCH_DTYPE)   # (never read here)
    out_s = np.zeros(4096, dtype=np.int32)
    out_c = np.zeros((4096, 3), dtype=np.int32)
    k = C.c_int64(-7)
    par = capi.CoverageParams(*params) if params is not None else None
    sp = capi.SelectParams(*sel) if sel is not None else None
    rp = C.c_void_p(LAB.ctypes.data + 5) if overlap else C.c_void_p(RES.ctypes.data)
    front = (None, C.c_void_p(LAB.ctypes.data) if labels else None, width, height, 0, None,
             C.c_void_p(rec.ctypes.data) if matches else None, n, on_device, 0, C.byref(par) if par is not None else None)
    cp = out_c.ctypes.data_as(C.POINTER(C.c_int32)) if counts else None
    if select:
        return capi.lib().fdcm_matches_select(*front, C.byref(sp) if sp is not None else None,
                                              out_s.ctypes.data_as(C.POINTER(C.c_int32)) if selected else None, cp,
                                              C.byref(k) if n_out else None, rp if residual or overlap else None)
    return capi.lib().fdcm_matches_coverage(*front, cp, rp if residual or overlap else None)


def test_exports_declares_and_binds_the_entry_points(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    for name, nargs in (("fdcm_matches_coverage", 13), ("fdcm_matches_select", 16)):
        assert hasattr(lib, name) and name in bound and len(bound[name][2]) == nargs and bound[name][1] is C.c_int
    cov, sel = bound["fdcm_matches_coverage"][2], bound["fdcm_matches_select"][2]
    assert sel[:11] == cov[:11] and sel[-1] == cov[-1]
    assert cov[:6] == bound["fdcm_scene_coverage"][2][:6]                       # the coverage calls' leading arguments
    assert cov[6:10] == bound["fdcm_matches_detect"][2][2:6]                    # the match calls' matches, n, on_device, tmpl_index_base
    assert sel[10:] == bound["fdcm_scene_select"][2][9:]                        # params, sel and the outputs
    root = os.path.join(os.path.dirname(capi.LIB_PATH), "..")
    with open(os.path.join(root, "include", "fdcm.h")) as f:
        header = f.read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, tail in (("fdcm_matches_coverage", ["params", "counts_out", "residual_out"]),
                       ("fdcm_matches_select", ["params", "sel", "selected_out", "counts_out", "n_out", "residual_out"])):
        decl = re.search(r"int %s\((.*?)\);" % name, plain, flags=re.S)
        names = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
        assert names[:10] == ["fm", "labels", "width", "height", "labels_on_device", "templates", "matches", "n", "matches_on_device",
                              "tmpl_index_base"] and names[10:] == tail
    assert "Match lists: scene coverage and selection" in header and "tests/match_coverage_ref.py" in header
    with open(os.path.join(root, "openfdcm_amd", "csrc", "fdcm_internal.h")) as f:
        internal = f.read()
    assert "run_matches_coverage" in internal and "run_matches_select" in internal and "FDCM_COVERAGE_PART" in internal
    with open(os.path.join(root, "README.md")) as f:
        assert "Match lists: scene coverage and selection" in f.read()
    with open(os.path.join(root, "DESIGN.md")) as f:
        assert "## 33. Match lists: scene coverage and selection" in f.read()


def test_python_signatures_and_defaults(capi):
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap
    p = inspect.signature(fd.match_coverage).parameters
    assert list(p) == ["featuremap", "labels", "templates", "matches", "radius", "bin_tolerance", "margin", "return_residual", "device_ptr", "n"]
    q = inspect.signature(fd.select_matches).parameters
    assert list(q) == ["featuremap", "labels", "templates", "matches", "radius", "bin_tolerance", "margin", "min_coverage", "min_new",
                       "min_pixels", "max_selected", "return_residual", "device_ptr", "n"]
    for s in (p, q):
        assert s["radius"].default == 2 and s["bin_tolerance"].default == 1 and s["margin"].default is None
        assert s["return_residual"].default is False and s["device_ptr"].default is None and s["n"].default == 0
    assert q["min_coverage"].default == 0.0 and q["min_new"].default == 0.5 and q["min_pixels"].default == 1 and q["max_selected"].default == 1024
    assert "detect_matches(.., overlap=1.0)" in fd.select_matches.__doc__ and "sort_matches(penalize(..))" in fd.select_matches.__doc__
    m = inspect.signature(DeviceFeatureMap.select_matches).parameters
    assert list(m)[:4] == ["self", "labels", "templates", "matches"] and m["matches"].default is None and m["tmpl_index_base"].default == 0
    assert list(inspect.signature(DeviceFeatureMap.match_coverage).parameters)[:4] == ["self", "labels", "templates", "matches"]
    # the siblings are as they were
    assert list(inspect.signature(fd.scene_select).parameters)[:4] == ["featuremap", "labels", "templates", "poses"]
    assert len({s[0]: s for s in capi.SYMBOLS}["fdcm_scene_coverage"][2]) == 12 and len({s[0]: s for s in capi.SYMBOLS}["fdcm_scene_select"][2]) == 15


def test_a_match_list_indexed_by_a_selection_is_a_match_list(capi):
    import openfdcm_amd as fd
    rec = np.zeros(6, dtype=capi.MATCH_DTYPE)
    rec["tmpl_idx"] = np.arange(6)
    rec["score"] = np.arange(6) * 0.5
    ml = fd.MatchList(rec)
    for sel in (np.int32([4, 1]), np.zeros(0, dtype=np.int32), np.int64([0, 5, 5])):
        parts = ml[sel]
        assert isinstance(parts, fd.MatchList) and len(parts) == len(sel) and parts.records().tobytes() == rec[sel].tobytes()
    ml.append(ml[0])                                                             # a restructured list
    assert [m.tmpl_idx for m in ml[np.int32([6, 2])]] == [0, 2]
    assert ml[2].tmpl_idx == 2 and isinstance(ml[1:3], fd.MatchList) and ml[np.int32(3)].tmpl_idx == 3   # the other forms are as they were


@pytest.mark.parametrize("select", [False, True], ids=["coverage", "select"])
def test_valid_arguments_reach_the_handles(capi, select):
    top = 1 << 16 if select else 1 << 20
    for n in (0, 1, top):
        for params in [(0, 0, 0), (32, 0, 4096)]:
            assert _call(capi, select, n=n, params=params, sel=(1000, 1000, 1 << 24, 4096), width=4096, height=4096, residual=True) == EINVAL
            assert "null featuremap/templates" in _err(capi)
    assert _call(capi, select, n=5, matches=False) == EINVAL and "null featuremap/templates" in _err(capi)   # NULL, on_device 0: the last search
    assert _call(capi, select, n=0, matches=False, on_device=1) == EINVAL and "null featuremap/templates" in _err(capi)


@pytest.mark.parametrize("select", [False, True], ids=["coverage", "select"])
def test_every_refusal_is_einval_with_its_message(capi, select):
    assert _call(capi, select, n=-1) == EINVAL and "n is negative" in _err(capi)
    if select:
        assert _call(capi, select, n=(1 << 16) + 1) == EINVAL and "n must be at most 2^16" in _err(capi) and "fdcm_matches_detect first" in _err(capi)
    else:
        assert _call(capi, select, n=(1 << 20) + 1) == EINVAL and "n must be at most 2^20" in _err(capi)
    for v in (-1, 2):
        assert _call(capi, select, on_device=v) == EINVAL and "on_device must be 0 or 1" in _err(capi)
    assert _call(capi, select, matches=False, on_device=1) == EINVAL and "matches is null" in _err(capi)
    assert _call(capi, select, params=None) == EINVAL and "params is null" in _err(capi)
    for r in (-1, 33):
        assert _call(capi, select, params=(r, 1, 2)) == EINVAL and "radius must be in [0, 32]" in _err(capi)
    assert _call(capi, select, params=(2, -1, 2)) == EINVAL and "bin_tolerance must be in [0, m / 2]" in _err(capi)
    for mg in (-1, 4097):
        assert _call(capi, select, params=(2, 1, mg)) == EINVAL and "margin must be in [0, 4096]" in _err(capi)
    assert _call(capi, select, labels=False) == EINVAL and "labels is null" in _err(capi)
    for w, h in [(0, 12), (16, 0), (4097, 12), (16, 4097), (-1, 12)]:
        assert _call(capi, select, width=w, height=h) == EINVAL and "width and height must be in [1, 4096]" in _err(capi)
    assert _call(capi, select, overlap=True) == EINVAL and "residual_out must not overlap labels" in _err(capi)
    if not select:
        assert _call(capi, select, counts=False) == EINVAL and "counts_out is null" in _err(capi)
        assert _call(capi, select, n=0, counts=False) == EINVAL and "null featuremap/templates" in _err(capi)   # n = 0 writes no counts
        return
    assert _call(capi, select, sel=None) == EINVAL and "sel is null" in _err(capi)
    for v in (-1, 1001):
        assert _call(capi, select, sel=(v, 500, 1, 8)) == EINVAL and "min_coverage_permille must be in [0, 1000]" in _err(capi)
        assert _call(capi, select, sel=(0, v, 1, 8)) == EINVAL and "min_new_permille must be in [0, 1000]" in _err(capi)
    for v in (0, -1, (1 << 24) + 1):
        assert _call(capi, select, sel=(0, 500, v, 8)) == EINVAL and "min_pixels must be in [1, 2^24]" in _err(capi)
    for v in (0, -1, 4097):
        assert _call(capi, select, sel=(0, 500, 1, v)) == EINVAL and "max_selected must be in [1, 4096]" in _err(capi)
    assert _call(capi, select, selected=False) == EINVAL and "selected_out is null" in _err(capi)
    assert _call(capi, select, counts=False) == EINVAL and "counts_out is null" in _err(capi)
    assert _call(capi, select, n_out=False) == EINVAL and "n_out is null" in _err(capi)
    # in the order of the section: the list, the parameters and the image, then sel, then the outputs, then the handles
    assert _call(capi, select, n=-1, params=None, sel=None, labels=False) == EINVAL and "n is negative" in _err(capi)
    assert _call(capi, select, on_device=3, params=None) == EINVAL and "on_device" in _err(capi)
    assert _call(capi, select, sel=None, width=0) == EINVAL and "width and height" in _err(capi)
    assert _call(capi, select, sel=None, selected=False, overlap=True) == EINVAL and "sel is null" in _err(capi)
    assert _call(capi, select, n_out=False, overlap=True) == EINVAL and "n_out is null" in _err(capi)
