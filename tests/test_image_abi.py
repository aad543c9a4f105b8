"""CPU-only checks of the image entry points of the C ABI (include/fdcm.h, "feature maps from images"): the library exports
them with the declared signatures, and every argument error is FDCM_EINVAL with a message before any device work -- no call
here reaches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import ROOT

EINVAL = -1
NEW_SYMBOLS = {
    "fdcm_edge_labels": 7, "fdcm_featuremap_build_image": 11, "fdcm_featuremap_rebuild_image": 8,
    "fdcm_featuremap_build_labels": 9, "fdcm_featuremap_rebuild_labels": 6, "fdcm_featuremap_build_image_staged": 12,
}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def test_exports_the_image_entry_points_as_declared(capi):
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
        for p, ct in zip(params, bound[name][2]):   # pointers bind as pointers, 64-bit sizes as c_int64, float as c_float
            if "*" in p:
                assert ct is C.c_void_p or issubclass(ct, C._Pointer), (name, p, ct)
            elif p.startswith("int64_t"):
                assert ct is C.c_int64, (name, p, ct)
            elif p.startswith("float"):
                assert ct is C.c_float, (name, p, ct)
            else:
                assert p.startswith("int ") and ct is C.c_int, (name, p, ct)


IMG = np.zeros((8, 10), dtype=np.uint8)


def _build_image(capi, image=IMG, width=10, height=8, stride=10, on_device=0, threshold=60, border=0, depth=6, distance=0,
                 out=True):
    h = C.c_void_p(0xdead)
    p = C.c_void_p(image.ctypes.data) if image is not None else None
    rc = capi.lib().fdcm_featuremap_build_image(p, width, height, stride, on_device, threshold, border, depth, 5.0, distance,
                                                C.byref(h) if out else None)
    if out and rc != 0:
        assert h.value is None          # a failed build hands out no handle
    return rc


@pytest.mark.parametrize("kw,what", [
    (dict(image=None), "image is null"),
    (dict(out=False), "out is null"),
    (dict(threshold=0), "threshold"), (dict(threshold=-5), "threshold"), (dict(threshold=1443), "threshold"),
    (dict(border=-1), "border"),
    (dict(width=0), "width and height"), (dict(height=0), "width and height"), (dict(width=-4), "width and height"),
    (dict(width=4097, stride=4097), "4096"), (dict(height=4097), "4096"),
    (dict(width=4000, stride=4000, border=49), "4096"), (dict(height=4096, border=1), "4096"),
    (dict(stride=9), "row_stride"),
    (dict(depth=256), "255"), (dict(depth=100000), "255"), (dict(depth=-1), "depth"),
    (dict(distance=3), "distance"),
    (dict(on_device=2), "on_device"),
])
def test_build_image_argument_errors(capi, kw, what):
    assert _build_image(capi, **kw) == EINVAL
    assert what in _err(capi), _err(capi)


def test_staged_hook_checks_stop_after_and_the_rest(capi):
    lib = capi.lib()
    h = C.c_void_p()
    p = C.c_void_p(IMG.ctypes.data)
    for stop in (0, 4, -1):
        assert lib.fdcm_featuremap_build_image_staged(p, 10, 8, 10, 0, 60, 0, 6, 5.0, 0, stop, C.byref(h)) == EINVAL
        assert "stop_after" in _err(capi)
    assert lib.fdcm_featuremap_build_image_staged(p, 10, 8, 10, 0, 0, 0, 6, 5.0, 0, 1, C.byref(h)) == EINVAL
    assert "threshold" in _err(capi)
    assert lib.fdcm_featuremap_build_image_staged(None, 10, 8, 10, 0, 60, 0, 6, 5.0, 0, 1, C.byref(h)) == EINVAL
    assert "null" in _err(capi)


def test_rebuild_argument_errors(capi):
    lib = capi.lib()
    p = C.c_void_p(IMG.ctypes.data)
    assert lib.fdcm_featuremap_rebuild_image(None, p, 10, 8, 10, 0, 60, 0) == EINVAL
    assert "featuremap is null" in _err(capi)
    assert lib.fdcm_featuremap_rebuild_labels(None, p, 10, 8, 0, 0) == EINVAL
    assert "featuremap is null" in _err(capi)


def test_labels_argument_errors(capi):
    lib = capi.lib()
    h = C.c_void_p()
    p = C.c_void_p(IMG.ctypes.data)
    build = lambda *a: lib.fdcm_featuremap_build_labels(*a, C.byref(h))
    assert build(None, 10, 8, 0, 0, 6, 5.0, 0) == EINVAL and "labels is null" in _err(capi)
    assert build(p, 0, 8, 0, 0, 6, 5.0, 0) == EINVAL and "width and height" in _err(capi)
    assert build(p, 10, 5000, 0, 0, 6, 5.0, 0) == EINVAL and "4096" in _err(capi)
    assert build(p, 10, 8, 0, -2, 6, 5.0, 0) == EINVAL and "border" in _err(capi)
    assert build(p, 10, 8, 0, 0, 300, 5.0, 0) == EINVAL and "255" in _err(capi)
    assert build(p, 10, 8, 0, 0, 6, 5.0, 9) == EINVAL and "distance" in _err(capi)
    assert lib.fdcm_featuremap_build_labels(p, 10, 8, 0, 0, 6, 5.0, 0, None) == EINVAL and "out is null" in _err(capi)


def test_edge_labels_argument_errors(capi):
    lib = capi.lib()
    out = np.zeros_like(IMG)
    p, q = C.c_void_p(IMG.ctypes.data), C.c_void_p(out.ctypes.data)
    assert lib.fdcm_edge_labels(None, 10, 8, 10, 6, 60, q) == EINVAL and "image is null" in _err(capi)
    assert lib.fdcm_edge_labels(p, 10, 8, 10, 6, 60, None) == EINVAL and "labels_out is null" in _err(capi)
    assert lib.fdcm_edge_labels(p, 10, 8, 9, 6, 60, q) == EINVAL and "row_stride" in _err(capi)
    assert lib.fdcm_edge_labels(p, 10, 8, 10, 6, 0, q) == EINVAL and "threshold" in _err(capi)
    assert lib.fdcm_edge_labels(p, 10, 8, 10, 6, 1443, q) == EINVAL and "threshold" in _err(capi)
    assert lib.fdcm_edge_labels(p, 10, 8, 10, 0, 60, q) == EINVAL and "depth" in _err(capi)
    assert lib.fdcm_edge_labels(p, 10, 8, 10, 256, 60, q) == EINVAL and "255" in _err(capi)
    assert lib.fdcm_edge_labels(p, 0, 8, 10, 6, 60, q) == EINVAL and "width and height" in _err(capi)
    assert lib.fdcm_edge_labels(p, 5000, 8, 5000, 6, 60, q) == EINVAL and "4096" in _err(capi)


def test_python_layer_rejects_other_arrays(capi):
    import openfdcm_amd
    with pytest.raises(ValueError):
        openfdcm_amd.edge_labels(np.zeros((4, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        openfdcm_amd.edge_labels(np.zeros((4, 4, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        openfdcm_amd.DeviceFeatureMap.build_image(np.zeros(16, dtype=np.uint8), 60)
