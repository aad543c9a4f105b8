"""CPU-only checks of the _ex image entry points of the C ABI (include/fdcm.h, "edges with smoothing, hysteresis and a minimum
chain length"), in the manner of test_image_abi.py: exported as declared and bound, and every argument error is FDCM_EINVAL
with a message before any device work -- no call here reaches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import ROOT

EINVAL = -1
NEW_SYMBOLS = {"fdcm_edge_labels_ex": 7, "fdcm_featuremap_build_image_ex": 11, "fdcm_featuremap_rebuild_image_ex": 8}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def test_exports_the_ex_entry_points_as_declared(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "fdcm.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(lib, name), name
        assert name in bound, name
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        assert len(params) == nargs == len(bound[name][2]), (name, params)
        for p, ct in zip(params, bound[name][2]):
            if "fdcm_edge_params*" in p:
                assert p.startswith("const ") and ct is C.POINTER(capi.EdgeParams), (name, p, ct)
            elif "*" in p:
                assert ct is C.c_void_p or issubclass(ct, C._Pointer), (name, p, ct)
            elif p.startswith("int64_t"):
                assert ct is C.c_int64, (name, p, ct)
            elif p.startswith("float"):
                assert ct is C.c_float, (name, p, ct)
            else:
                assert p.startswith("int ") and ct is C.c_int, (name, p, ct)


def test_the_struct_is_the_headers(capi):
    header = open(os.path.join(ROOT, "include", "fdcm.h")).read()
    body = re.search(r"typedef struct fdcm_edge_params \{(.*?)\} fdcm_edge_params;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("int32_t", "").split(",")]
    assert names == ["smooth", "low", "high", "min_pixels"] == [f[0] for f in capi.EdgeParams._fields_]
    assert all(f[1] is C.c_int32 for f in capi.EdgeParams._fields_) and C.sizeof(capi.EdgeParams) == 16


IMG = np.zeros((8, 10), dtype=np.uint8)
GOOD = dict(smooth=1, low=20, high=60, min_pixels=8)


def _params(capi, kw):
    if kw.get("params", True) is None:
        return None
    v = dict(GOOD, **{k: kw[k] for k in GOOD if k in kw})
    return C.byref(capi.EdgeParams(v["smooth"], v["low"], v["high"], v["min_pixels"]))


def _build(capi, image=IMG, width=10, height=8, stride=10, on_device=0, border=0, depth=6, distance=0, out=True, **kw):
    h = C.c_void_p(0xdead)
    p = C.c_void_p(image.ctypes.data) if image is not None else None
    rc = capi.lib().fdcm_featuremap_build_image_ex(p, width, height, stride, on_device, _params(capi, kw), border, depth, 5.0, distance,
                                                   C.byref(h) if out else None)
    if out and rc != 0:
        assert h.value is None          # a failed build hands out no handle
    return rc


PARAM_ERRORS = [
    (dict(params=None), "params is null"),
    (dict(smooth=-1), "smooth"), (dict(smooth=3), "smooth"),
    (dict(low=0), "low"), (dict(low=-3), "low"), (dict(high=1443), "high"), (dict(low=61), "low"), (dict(low=1500, high=1500), "high"),
    (dict(min_pixels=0), "min_pixels"), (dict(min_pixels=-2), "min_pixels"),
]
SIBLING_ERRORS = [
    (dict(image=None), "image is null"),
    (dict(out=False), "out is null"),
    (dict(border=-1), "border"),
    (dict(width=0), "width and height"), (dict(height=0), "width and height"), (dict(width=-4), "width and height"),
    (dict(width=4097, stride=4097), "4096"), (dict(height=4097), "4096"),
    (dict(width=4000, stride=4000, border=49), "4096"), (dict(height=4096, border=1), "4096"),
    (dict(stride=9), "row_stride"),
    (dict(depth=256), "255"), (dict(depth=100000), "255"), (dict(depth=-1), "depth"),
    (dict(distance=3), "distance"),
    (dict(on_device=2), "on_device"),
]


@pytest.mark.parametrize("kw,what", PARAM_ERRORS + SIBLING_ERRORS, ids=lambda v: str(v))
def test_build_image_ex_argument_errors(capi, kw, what):
    assert _build(capi, **kw) == EINVAL
    assert what in _err(capi), _err(capi)


@pytest.mark.parametrize("kw,what", PARAM_ERRORS, ids=lambda v: str(v))
def test_edge_labels_ex_parameter_errors(capi, kw, what):
    lib = capi.lib()
    out = np.zeros_like(IMG)
    p, q = C.c_void_p(IMG.ctypes.data), C.c_void_p(out.ctypes.data)
    assert lib.fdcm_edge_labels_ex(p, 10, 8, 10, 6, _params(capi, kw), q) == EINVAL
    assert what in _err(capi), _err(capi)


def test_rebuild_ex_without_a_handle(capi):
    """(The handle is checked first; a rebuild's parameter errors need a handle, so tests/test_gpu_edge_ex.py has them.)"""
    p = C.c_void_p(IMG.ctypes.data)
    assert capi.lib().fdcm_featuremap_rebuild_image_ex(None, p, 10, 8, 10, 0, _params(capi, {}), 0) == EINVAL
    assert "featuremap is null" in _err(capi)


def test_edge_labels_ex_sibling_errors(capi):
    lib = capi.lib()
    out = np.zeros_like(IMG)
    p, q, e = C.c_void_p(IMG.ctypes.data), C.c_void_p(out.ctypes.data), _params(capi, {})
    assert lib.fdcm_edge_labels_ex(None, 10, 8, 10, 6, e, q) == EINVAL and "image is null" in _err(capi)
    assert lib.fdcm_edge_labels_ex(p, 10, 8, 10, 6, e, None) == EINVAL and "labels_out is null" in _err(capi)
    assert lib.fdcm_edge_labels_ex(p, 10, 8, 9, 6, e, q) == EINVAL and "row_stride" in _err(capi)
    assert lib.fdcm_edge_labels_ex(p, 10, 8, 10, 0, e, q) == EINVAL and "depth" in _err(capi)
    assert lib.fdcm_edge_labels_ex(p, 10, 8, 10, 256, e, q) == EINVAL and "255" in _err(capi)
    assert lib.fdcm_edge_labels_ex(p, 0, 8, 10, 6, e, q) == EINVAL and "width and height" in _err(capi)
    assert lib.fdcm_edge_labels_ex(p, 5000, 8, 5000, 6, e, q) == EINVAL and "4096" in _err(capi)


def test_python_layer(capi):
    import inspect

    import openfdcm_amd
    from openfdcm_amd.engine import DeviceFeatureMap
    for fn in (openfdcm_amd.edge_labels, DeviceFeatureMap.build_image, DeviceFeatureMap.rebuild_image, openfdcm_amd.build_image_featuremap):
        sig = inspect.signature(fn).parameters
        assert (sig["low"].default, sig["smooth"].default, sig["min_pixels"].default) == (None, 0, 1), fn
    img = np.zeros((8, 10), dtype=np.uint8)
    for opt in (dict(low=20), dict(smooth=1), dict(min_pixels=8)):
        for stop in (1, 2):
            with pytest.raises(ValueError, match="stop_after"):
                DeviceFeatureMap.build_image(img, 60, depth=6, stop_after=stop, **opt)
    with pytest.raises(openfdcm_amd._capi.FdcmError, match="low"):
        openfdcm_amd.edge_labels(img, depth=6, threshold=60, low=61)
    with pytest.raises(openfdcm_amd._capi.FdcmError, match="smooth"):
        DeviceFeatureMap.build_image(img, 60, depth=6, smooth=3)
    with pytest.raises(ValueError):
        openfdcm_amd.edge_labels(np.zeros((4, 4), dtype=np.float32), low=20)
