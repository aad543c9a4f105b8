"""CPU-only checks of the line-segment entry points of the C ABI (include/fdcm.h, "line segments from images"), in the manner
of test_edge_ex_abi.py: exported as declared and bound, and every argument error is FDCM_EINVAL with a message before any
device work -- no call here reaches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import ROOT

EINVAL = -1
NEW_SYMBOLS = {"fdcm_lines_from_labels": 8, "fdcm_lines_from_image": 10, "fdcm_lines_last_timing": 1}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def test_exports_the_line_entry_points_as_declared(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "fdcm.h")).read()
    structs = {"fdcm_edge_params*": capi.EdgeParams, "fdcm_line_params*": capi.LineParams, "fdcm_lines_timing*": capi.LinesTiming}
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(lib, name), name
        assert name in bound, name
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        assert len(params) == nargs == len(bound[name][2]), (name, params)
        for p, ct in zip(params, bound[name][2]):
            struct = [v for k, v in structs.items() if k in p]
            if struct:
                assert ct is C.POINTER(struct[0]), (name, p, ct)
            elif "float**" in p:
                assert ct is C.POINTER(C.POINTER(C.c_float)), (name, p, ct)
            elif "*" in p:
                assert ct is C.c_void_p or issubclass(ct, C._Pointer), (name, p, ct)
            elif p.startswith("int64_t"):
                assert ct is C.c_int64, (name, p, ct)
            else:
                assert p.startswith("int ") and ct is C.c_int, (name, p, ct)


def test_the_structs_are_the_headers(capi):
    header = open(os.path.join(ROOT, "include", "fdcm.h")).read()
    body = re.search(r"typedef struct fdcm_line_params \{(.*?)\} fdcm_line_params;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("int32_t", "").split(",")]
    assert names == ["bucket", "min_pixels", "min_length"] == [f[0] for f in capi.LineParams._fields_]
    assert all(f[1] is C.c_int32 for f in capi.LineParams._fields_) and C.sizeof(capi.LineParams) == 12
    body = re.search(r"typedef struct fdcm_lines_timing \{(.*?)\} fdcm_lines_timing;", header, re.S).group(1)
    floats = [n.strip() for n in re.search(r"float (.*?);", body, re.S).group(1).split(",")]
    assert floats + ["n_lines"] == [f[0] for f in capi.LinesTiming._fields_] and "int64_t n_lines;" in body


LAB = np.full((8, 10), 255, dtype=np.uint8)
GOOD_LINE = dict(bucket=4, min_pixels=8, min_length=8)
GOOD_EDGE = dict(smooth=1, low=20, high=60, edge_min_pixels=8)


def _line_params(capi, kw):
    if kw.get("params", True) is None:
        return None
    v = dict(GOOD_LINE, **{k: kw[k] for k in GOOD_LINE if k in kw})
    return C.byref(capi.LineParams(v["bucket"], v["min_pixels"], v["min_length"]))


def _edge_params(capi, kw):
    if kw.get("edge", True) is None:
        return None
    v = dict(GOOD_EDGE, **{k: kw[k] for k in GOOD_EDGE if k in kw})
    return C.byref(capi.EdgeParams(v["smooth"], v["low"], v["high"], v["edge_min_pixels"]))


def _outputs(kw):
    lines, n = C.POINTER(C.c_float)(), C.c_int64(-7)
    return lines, n, (C.byref(lines) if kw.get("lines", True) else None), (C.byref(n) if kw.get("n_lines", True) else None)


def _from_labels(capi, pixels=LAB, width=10, height=8, on_device=0, depth=6, **kw):
    lines, n, pl, pn = _outputs(kw)
    p = C.c_void_p(pixels.ctypes.data) if pixels is not None else None
    rc = capi.lib().fdcm_lines_from_labels(p, width, height, on_device, depth, _line_params(capi, kw), pl, pn)
    assert not lines and n.value == -7      # a refused call hands nothing out
    return rc


def _from_image(capi, pixels=LAB, width=10, height=8, stride=10, on_device=0, depth=6, **kw):
    lines, n, pl, pn = _outputs(kw)
    p = C.c_void_p(pixels.ctypes.data) if pixels is not None else None
    rc = capi.lib().fdcm_lines_from_image(p, width, height, stride, on_device, depth, _edge_params(capi, kw), _line_params(capi, kw), pl, pn)
    assert not lines and n.value == -7
    return rc


LINE_ERRORS = [
    (dict(params=None), "line params is null"),
    (dict(lines=False), "lines is null"), (dict(n_lines=False), "n_lines is null"),
    (dict(bucket=0), "bucket"), (dict(bucket=-1), "bucket"), (dict(bucket=7), "bucket"), (dict(bucket=31, depth=30), "bucket"),
    (dict(bucket=2, depth=1), "bucket"),
    (dict(min_pixels=1), "min_pixels"), (dict(min_pixels=0), "min_pixels"), (dict(min_pixels=65536), "min_pixels"),
    (dict(min_length=0), "min_length"), (dict(min_length=4097), "min_length"),
    (dict(width=0), "width and height"), (dict(height=0), "width and height"), (dict(width=-4), "width and height"),
    (dict(width=4097), "4096"), (dict(height=4097), "4096"),
    (dict(depth=0), "depth"), (dict(depth=-1), "depth"), (dict(depth=256), "255"), (dict(depth=100000), "255"),
    (dict(on_device=2), "on_device"),
]
EDGE_ERRORS = [
    (dict(pixels=None), "image is null"),
    (dict(stride=9), "row_stride"),
    (dict(edge=None), "params is null"),
    (dict(smooth=-1), "smooth"), (dict(smooth=3), "smooth"),
    (dict(low=0), "low"), (dict(high=1443), "high"), (dict(low=61), "low"),
    (dict(edge_min_pixels=0), "min_pixels"),
]


@pytest.mark.parametrize("kw,what", LINE_ERRORS + [(dict(pixels=None), "labels is null")], ids=lambda v: str(v))
def test_lines_from_labels_argument_errors(capi, kw, what):
    assert _from_labels(capi, **kw) == EINVAL
    assert what in _err(capi), _err(capi)


@pytest.mark.parametrize("kw,what", LINE_ERRORS + EDGE_ERRORS, ids=lambda v: str(v))
def test_lines_from_image_argument_errors(capi, kw, what):
    if "width" in kw:
        kw = dict(kw, stride=max(kw["width"], 10))
    assert _from_image(capi, **kw) == EINVAL
    assert what in _err(capi), _err(capi)


def test_the_largest_arguments_are_not_refused_for_their_size(capi):
    """bucket = m, min_pixels = 65535 and min_length = 4096 pass the checks: the call is refused for the null image behind them."""
    assert _from_image(capi, pixels=None, bucket=6, min_pixels=65535, min_length=4096) == EINVAL and "image is null" in _err(capi)
    assert _from_labels(capi, pixels=None, bucket=1, min_pixels=2, min_length=1) == EINVAL and "labels is null" in _err(capi)


def test_last_timing_without_a_destination(capi):
    assert capi.lib().fdcm_lines_last_timing(None) == EINVAL and "out is null" in _err(capi)


def test_python_layer(capi):
    import inspect

    import openfdcm_amd
    sig = inspect.signature(openfdcm_amd.lines_from_labels).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("depth", 30), ("bucket", 4), ("line_pixels", 8), ("line_length", 8)]
    sig = inspect.signature(openfdcm_amd.lines_from_image).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("depth", 30), ("threshold", 60), ("low", None), ("smooth", 0), ("min_pixels", 1),
                                                            ("bucket", 4), ("line_pixels", 8), ("line_length", 8)]
    img = np.zeros((8, 10), dtype=np.uint8)
    with pytest.raises(openfdcm_amd._capi.FdcmError, match="bucket"):
        openfdcm_amd.lines_from_labels(img, depth=6, bucket=7)
    with pytest.raises(openfdcm_amd._capi.FdcmError, match="min_pixels"):
        openfdcm_amd.lines_from_image(img, depth=6, line_pixels=1)
    with pytest.raises(openfdcm_amd._capi.FdcmError, match="low"):
        openfdcm_amd.lines_from_image(img, depth=6, threshold=60, low=61)
    for fn in (openfdcm_amd.lines_from_labels, openfdcm_amd.lines_from_image):
        with pytest.raises(ValueError):
            fn(np.zeros((4, 4), dtype=np.float32))
        with pytest.raises(ValueError):
            fn(np.zeros((4, 4, 3), dtype=np.uint8))
