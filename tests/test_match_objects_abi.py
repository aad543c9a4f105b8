"""Checks of the match lists with objects and hull shapes (include/fdcm.h, "Match lists: objects and hull shapes") that need no
device: the library exports the three entry points, the binding and the header know them, the Python names have the stated
signatures and defaults, and every argument check returns FDCM_EINVAL with its own message before any handle or device is
touched (the handles are NULL throughout: a late check would report them instead).  The labels are checked against the set, and
the span table's size after the pass: both need handles and are in tests/test_gpu_match_objects.py, with the empty inputs."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

EINVAL = -1
MATCH = np.dtype([("tmpl_idx", "<i4"), ("score", "<f4"), ("transform", "<f4", (6,))])
RECS = np.zeros(8, dtype=MATCH)
OBJ = np.zeros(4, dtype=np.int32)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def _detect(capi, matches=True, n=8, on_device=0, base=0, n_objects=2, max_score=(1.0, np.inf), min_matched=None, max_detections=64,
            permille=300, cross=800, margin=0, penalty=-1, tau=1.0, rescore=0, out=True, n_out=True):
    o, k = C.c_void_p(), C.c_int64(-7)
    ms = None if max_score is None else np.asarray(max_score, dtype=np.float32)
    mm = None if min_matched is None else np.asarray(min_matched, dtype=np.float32)
    return capi.lib().fdcm_matches_detect_objects(
        None, None, C.c_void_p(RECS.ctypes.data) if matches else None, n, on_device, base, OBJ.ctypes.data_as(C.POINTER(C.c_int32)), n_objects,
        capi.fptr(ms) if ms is not None else None, capi.fptr(mm) if mm is not None else None, max_detections, permille, cross, margin, penalty,
        tau, rescore, C.byref(o) if out else None, C.byref(k) if n_out else None, None, None, None)


def _spans(capi, matches=True, n=8, margin=0, offsets=True):
    off = np.zeros(9, dtype=np.int64)
    return capi.lib().fdcm_matches_footprint_spans(None, C.c_void_p(RECS.ctypes.data) if matches else None, n, 0, margin,
                                                   off.ctypes.data_as(C.POINTER(C.c_int64)) if offsets else None, None, None)


def _shapes(capi, matches=True, n=8, on_device=0, margin=0, offsets=True):
    off = np.zeros(9, dtype=np.int64)
    return capi.lib().fdcm_matches_shapes(None, None, C.c_void_p(RECS.ctypes.data) if matches else None, n, on_device, 0, margin,
                                          off.ctypes.data_as(C.POINTER(C.c_int64)) if offsets else None, None, None)


def test_exports_declares_and_binds_the_entry_points(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    root = os.path.join(os.path.dirname(capi.LIB_PATH), "..")
    with open(os.path.join(root, "include", "fdcm.h")) as f:
        header = f.read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args, tail in [("fdcm_matches_detect_objects", 22, ["rescore", "out", "n_out", "indices_out", "boxes_out", "matched_out"]),
                               ("fdcm_matches_footprint_spans", 8, ["margin", "row_offsets", "areas", "spans"]),
                               ("fdcm_matches_shapes", 10, ["margin", "row_offsets", "areas", "spans"])]:
        assert hasattr(lib, name) and name in bound and bound[name][1] is C.c_int and len(bound[name][2]) == n_args
        decl = re.search(r"int %s\((.*?)\);" % name, plain, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == n_args
        names = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
        assert names[-len(tail):] == tail
    assert "Match lists: objects and hull shapes" in header and "tests/match_objects_ref.py" in header
    assert "fdcm_matches_detect_objects" in header[header.index("Calls that honour the kind"):header.index("Span tables:")]
    with open(os.path.join(root, "README.md")) as f:
        assert "Match lists: objects and hull shapes" in f.read()
    with open(os.path.join(root, "DESIGN.md")) as f:
        assert "## 34. Match lists: objects and hull shapes" in f.read()


def test_python_signatures_and_defaults(capi):
    import openfdcm_amd as fd
    from openfdcm_amd import engine
    p = inspect.signature(fd.detect_matches_objects).parameters
    assert list(p)[:8] == ["featuremap", "templates", "matches", "objects", "max_score", "overlap", "cross_overlap", "max_detections"]
    assert p["objects"].default is None and p["max_score"].default == float("inf") and p["overlap"].default == 0.3
    assert p["cross_overlap"].default is None and p["min_matched"].default is None and p["max_detections"].default == 1024
    assert all(p[k].default is False for k in ("rescore", "return_indices", "return_boxes", "return_matched", "return_objects"))
    assert p["device_ptr"].default is None and p["n"].default == 0
    assert list(inspect.signature(fd.match_footprint_spans).parameters) == ["templates", "matches", "margin"]
    q = inspect.signature(engine.DeviceFeatureMap.detect_matches_objects).parameters
    assert q["overlap_permille"].default == 300 and q["cross_permille"].default is None
    assert "match_shapes" in dir(engine.DeviceFeatureMap) and callable(engine.match_footprint_spans)
    # the sibling is as it was
    assert len({s[0]: s for s in capi.SYMBOLS}["fdcm_matches_detect"][2]) == 19


def test_valid_arguments_reach_the_handles(capi):
    for kw in [dict(), dict(n=0), dict(matches=False, n=0, on_device=1), dict(matches=False, n=5), dict(n_objects=1, max_score=(0.0,)),
               dict(n_objects=256, max_score=[1.0] * 256), dict(min_matched=(0.0, 1.0)), dict(cross=0), dict(cross=1000), dict(permille=0),
               dict(max_detections=1), dict(max_detections=4096), dict(margin=4096), dict(penalty=1, tau=-2.5), dict(rescore=1)]:
        assert _detect(capi, **kw) == EINVAL and "null featuremap/templates" in _err(capi), kw
    assert _spans(capi, margin=4096) == EINVAL and "templates is null" in _err(capi)
    assert _shapes(capi, margin=4096) == EINVAL and "null featuremap/templates" in _err(capi)


def test_every_refused_argument_is_einval_with_its_message(capi):
    big = (1 << 22) + 1
    for call in (_detect, _shapes):
        assert call(capi, n=-1) == EINVAL and "n is negative" in _err(capi)
        assert call(capi, n=big) == EINVAL and "n must be at most 2^22" in _err(capi)
        assert call(capi, matches=False, n=3, on_device=1) == EINVAL and "matches is null" in _err(capi)
        assert call(capi, on_device=2) == EINVAL and "on_device must be 0 or 1" in _err(capi)
    for v in (0, -1, 257):
        assert _detect(capi, n_objects=v) == EINVAL and "n_objects must be in [1, 256]" in _err(capi)
    assert _detect(capi, max_score=None) == EINVAL and "max_score is null" in _err(capi)
    for v in ((1.0, -1.0), (float("nan"), 1.0), (1.0, -np.inf)):
        assert _detect(capi, max_score=v) == EINVAL and "max_score must be >= 0" in _err(capi)
    for v in ((0.5, -0.1), (1.1, 0.0), (0.0, float("nan"))):
        assert _detect(capi, min_matched=v) == EINVAL and "min_matched must be in [0, 1]" in _err(capi)
    for v in (0, -1, 4097):
        assert _detect(capi, max_detections=v) == EINVAL and "max_detections must be in [1, 4096]" in _err(capi)
    for v in (-1, 1001):
        assert _detect(capi, permille=v) == EINVAL and "overlap_permille must be in [0, 1000]" in _err(capi)
        assert _detect(capi, cross=v) == EINVAL and "cross_permille must be in [0, 1000]" in _err(capi)
    for v in (-1, 4097):
        for call in (_detect, _spans, _shapes):
            assert call(capi, margin=v) == EINVAL and "margin must be in [0, 4096]" in _err(capi)
    for v in (-2, 2, 7):
        assert _detect(capi, penalty=v) == EINVAL and "unknown penalty" in _err(capi)
    for v in (float("nan"), float("inf")):
        assert _detect(capi, tau=v) == EINVAL and "tau must be finite" in _err(capi)
    for v in (-1, 2):
        assert _detect(capi, rescore=v) == EINVAL and "rescore must be 0 or 1" in _err(capi)
    assert _detect(capi, out=False) == EINVAL and "null output" in _err(capi)
    assert _detect(capi, n_out=False) == EINVAL and "null output" in _err(capi)
    assert _spans(capi, n=-1) == EINVAL and "n is negative" in _err(capi)
    assert _spans(capi, n=big) == EINVAL and "n must be at most 2^22" in _err(capi)
    assert _spans(capi, matches=False) == EINVAL and "matches is null" in _err(capi)
    for call in (_spans, _shapes):
        assert call(capi, offsets=False) == EINVAL and "row_offsets is null" in _err(capi)
    # in the order of the section: the list, the objects' arrays, the limits, the outputs, then the handles
    assert _detect(capi, n=-1, n_objects=0, out=False) == EINVAL and "n is negative" in _err(capi)
    assert _detect(capi, n_objects=0, max_detections=0, out=False) == EINVAL and "n_objects" in _err(capi)
    assert _detect(capi, cross=2000, rescore=5, out=False) == EINVAL and "cross_permille" in _err(capi)
