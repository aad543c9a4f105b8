"""Checks of the calls on match lists (include/fdcm.h, "Match lists") that need no device: the library exports the three entry
points, the binding and the header know them, the Python names have the stated signatures and defaults, and every argument
check returns FDCM_EINVAL with its own message before any handle or device is touched (the handles are NULL throughout: a late
check would report them instead).  The empty inputs need handles, which a process without a device cannot make: they are in
test_gpu_matches.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

EINVAL = -1
MATCH = np.dtype([("tmpl_idx", "<i4"), ("score", "<f4"), ("transform", "<f4", (6,))])
RECS = np.zeros(8, dtype=MATCH)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def _detect(capi, matches=True, n=8, on_device=0, base=0, max_score=np.inf, max_detections=64, permille=300, margin=0, penalty=-1, tau=1.0,
            min_matched=0.0, rescore=0, out=True, n_out=True):
    o, k = C.c_void_p(), C.c_int64(-7)
    return capi.lib().fdcm_matches_detect(None, None, C.c_void_p(RECS.ctypes.data) if matches else None, n, on_device, base, max_score,
                                          max_detections, permille, margin, penalty, tau, min_matched, rescore, C.byref(o) if out else None,
                                          C.byref(k) if n_out else None, None, None, None)


def _verify(capi, matches=True, n=8, on_device=0, outputs=(True, True, True)):
    s, f, c = np.zeros(8, dtype=np.float32), np.zeros(8, dtype=np.float32), np.zeros(8, dtype=np.float32)
    return capi.lib().fdcm_matches_verify(None, None, C.c_void_p(RECS.ctypes.data) if matches else None, n, on_device, 0,
                                          capi.fptr(s) if outputs[0] else None, capi.fptr(f) if outputs[1] else None,
                                          capi.fptr(c) if outputs[2] else None)


def _foot(capi, matches=True, n=8, margin=0, boxes=True):
    b = np.zeros((8, 4), dtype=np.int32)
    return capi.lib().fdcm_matches_footprints(None, C.c_void_p(RECS.ctypes.data) if matches else None, n, 0, margin,
                                              b.ctypes.data_as(C.POINTER(C.c_int32)) if boxes else None)


def test_exports_declares_and_binds_the_entry_points(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    root = os.path.join(os.path.dirname(capi.LIB_PATH), "..")
    with open(os.path.join(root, "include", "fdcm.h")) as f:
        header = f.read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args, tail in [("fdcm_matches_footprints", 6, ["margin", "boxes_out"]),
                               ("fdcm_matches_verify", 9, ["scores_out", "fractions_out", "costs_out"]),
                               ("fdcm_matches_detect", 19, ["rescore", "out", "n_out", "indices_out", "boxes_out", "matched_out"])]:
        assert hasattr(lib, name) and name in bound and bound[name][1] is C.c_int and len(bound[name][2]) == n_args
        decl = re.search(r"int %s\((.*?)\);" % name, plain, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == n_args
        names = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
        assert names[-len(tail):] == tail
    assert "Match lists" in header and "tests/match_ref.py" in header and "s(r) is not r.score" in header
    with open(os.path.join(root, "openfdcm_amd", "csrc", "fdcm_internal.h")) as f:
        assert "run_matches" in f.read()
    with open(os.path.join(root, "README.md")) as f:
        assert "detect_matches" in f.read()
    with open(os.path.join(root, "DESIGN.md")) as f:
        assert "## 31. Match lists" in f.read()


def test_python_signatures_and_defaults(capi):
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap
    p = inspect.signature(fd.detect_matches).parameters
    assert list(p) == ["featuremap", "templates", "matches", "max_score", "overlap", "max_detections", "penalty", "margin", "line_caps",
                       "min_matched", "rescore", "return_indices", "return_boxes", "return_matched", "device_ptr", "n"]
    assert p["max_score"].default == float("inf") and p["overlap"].default == 0.3 and p["max_detections"].default == 1024
    assert p["penalty"].default is None and p["margin"].default == 0 and p["line_caps"].default is None and p["min_matched"].default == 0.0
    assert all(p[k].default is False for k in ("rescore", "return_indices", "return_boxes", "return_matched"))
    assert p["device_ptr"].default is None and p["n"].default == 0
    assert list(inspect.signature(fd.verify_matches).parameters) == ["featuremap", "templates", "matches", "line_caps", "device_ptr", "n"]
    assert list(inspect.signature(fd.match_footprints).parameters) == ["templates", "matches", "margin"]
    q = inspect.signature(DeviceFeatureMap.detect_matches).parameters
    assert q["overlap_permille"].default == 300 and q["max_detections"].default == 1024 and q["matches"].default is None
    assert "verify_matches" in dir(DeviceFeatureMap)
    # the siblings are as they were
    assert list(inspect.signature(fd.topk).parameters) == ["fm", "templates", "k", "penalty", "tau", "tmpl_index_base", "device_ptr", "n"]
    assert len({s[0]: s for s in capi.SYMBOLS}["fdcm_topk"][2]) == 10


def test_valid_arguments_reach_the_handles(capi):
    """The bounds are inclusive: with them the call goes on to the (null) handles."""
    for kw in [dict(), dict(n=0), dict(matches=False, n=0, on_device=1), dict(matches=False, n=5), dict(max_score=0.0), dict(max_detections=1),
               dict(max_detections=4096), dict(permille=0), dict(permille=1000), dict(margin=4096), dict(penalty=0), dict(penalty=1, tau=-2.5),
               dict(min_matched=1.0), dict(rescore=1), dict(on_device=1), dict(base=-5)]:
        assert _detect(capi, **kw) == EINVAL and "null featuremap/templates" in _err(capi), kw
    assert _verify(capi) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _verify(capi, outputs=(False, False, True)) == EINVAL and "null featuremap/templates" in _err(capi)
    assert _foot(capi, margin=4096) == EINVAL and "templates is null" in _err(capi)
    assert _foot(capi, matches=False, n=0, boxes=False) == EINVAL and "templates is null" in _err(capi)


def test_every_refused_argument_is_einval_with_its_message(capi):
    big = (1 << 22) + 1
    for call in (_detect, _verify):
        assert call(capi, n=-1) == EINVAL and "n is negative" in _err(capi)
        assert call(capi, n=big) == EINVAL and "n must be at most 2^22" in _err(capi)
        assert call(capi, matches=False, n=3, on_device=1) == EINVAL and "matches is null" in _err(capi)
        assert call(capi, on_device=2) == EINVAL and "on_device must be 0 or 1" in _err(capi)
    for v in (-1.0, float("nan"), -np.inf):
        assert _detect(capi, max_score=v) == EINVAL and "max_score must be >= 0" in _err(capi)
    for v in (0, -1, 4097):
        assert _detect(capi, max_detections=v) == EINVAL and "max_detections must be in [1, 4096]" in _err(capi)
    for v in (-1, 1001):
        assert _detect(capi, permille=v) == EINVAL and "overlap_permille must be in [0, 1000]" in _err(capi)
    for v in (-1, 4097):
        assert _detect(capi, margin=v) == EINVAL and "margin must be in [0, 4096]" in _err(capi)
        assert _foot(capi, margin=v) == EINVAL and "margin must be in [0, 4096]" in _err(capi)
    for v in (-2, 2, 7):
        assert _detect(capi, penalty=v) == EINVAL and "unknown penalty" in _err(capi)
    for v in (float("nan"), float("inf")):
        assert _detect(capi, tau=v) == EINVAL and "tau must be finite" in _err(capi)
    for v in (-0.1, 1.1, float("nan")):
        assert _detect(capi, min_matched=v) == EINVAL and "min_matched must be in [0, 1]" in _err(capi)
    for v in (-1, 2):
        assert _detect(capi, rescore=v) == EINVAL and "rescore must be 0 or 1" in _err(capi)
    assert _detect(capi, out=False) == EINVAL and "null output" in _err(capi)
    assert _detect(capi, n_out=False) == EINVAL and "null output" in _err(capi)
    assert _verify(capi, outputs=(False, False, False)) == EINVAL and "every output is null" in _err(capi)
    assert _foot(capi, n=-1) == EINVAL and "n is negative" in _err(capi)
    assert _foot(capi, n=big) == EINVAL and "n must be at most 2^22" in _err(capi)
    assert _foot(capi, matches=False) == EINVAL and "matches is null" in _err(capi)
    assert _foot(capi, boxes=False) == EINVAL and "boxes_out is null" in _err(capi)
    # in the order of the section: the list, the parameters, the outputs, then the handles
    assert _detect(capi, n=-1, max_score=-1.0, out=False) == EINVAL and "n is negative" in _err(capi)
    assert _detect(capi, max_score=-1.0, max_detections=0, out=False) == EINVAL and "max_score" in _err(capi)
    assert _detect(capi, rescore=5, out=False) == EINVAL and "rescore" in _err(capi)
