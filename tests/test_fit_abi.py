"""Checks of fdcm_matches_fit (include/fdcm.h, "Match lists: pose fit") that need no device: the library exports the entry point,
the binding and the header know it, the parameter struct has its size, the Python names have the stated signatures and
defaults, and every argument check returns FDCM_EINVAL with its own message before any handle or device is touched (the
handles are NULL throughout: a late check would report them instead).  A process without a device cannot make the handles
the call needs: there the way to the call ends in FDCM_EHIP (a fresh process with every device hidden).  The empty inputs
need handles: they are in test_gpu_fit.py."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

EINVAL = -1
MATCH = np.dtype([("tmpl_idx", "<i4"), ("score", "<f4"), ("transform", "<f4", (6,))])
RECS = np.zeros(8, dtype=MATCH)
OUT = np.zeros(8, dtype=MATCH)
LAB = np.zeros(4096 * 4096, dtype=np.uint8)   # the largest image the call takes (never read here)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def _fit(capi, matches=True, n=8, on_device=0, params=(3, 1, 3), fit=(2, 8, 1e-3, 3.0, 0.1), labels=True, width=16, height=12, out=True,
         out_on_device=0):
    par = capi.CoverageParams(*params) if params is not None else None
    fp = capi.FitParams(*fit) if fit is not None else None
    info, rms = np.zeros((8, 4), dtype=np.int32), np.zeros((8, 2), dtype=np.float32)
    return capi.lib().fdcm_matches_fit(None, C.c_void_p(LAB.ctypes.data) if labels else None, width, height, 0, None,
                                       C.c_void_p(RECS.ctypes.data) if matches else None, n, on_device, 0,
                                       C.byref(par) if par is not None else None, C.byref(fp) if fp is not None else None,
                                       C.c_void_p(OUT.ctypes.data) if out else None, out_on_device,
                                       info.ctypes.data_as(C.POINTER(C.c_int32)), capi.fptr(rms))


def test_exports_declares_and_binds_the_entry_point(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    root = os.path.join(os.path.dirname(capi.LIB_PATH), "..")
    with open(os.path.join(root, "include", "fdcm.h")) as f:
        header = f.read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    name = "fdcm_matches_fit"
    assert hasattr(lib, name) and name in bound and bound[name][1] is C.c_int and len(bound[name][2]) == 16
    decl = re.search(r"int %s\((.*?)\);" % name, plain, flags=re.S)
    assert decl and len(decl.group(1).split(",")) == 16
    names = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert names == ["fm", "labels", "width", "height", "labels_on_device", "templates", "matches", "n", "matches_on_device",
                     "tmpl_index_base", "params", "fit", "out", "out_on_device", "info_out", "rms_out"]
    assert header.index("Match lists: refinement") < header.index("Match lists: pose fit") < header.index("host-side self checks")
    assert "tests/fit_ref.py" in header and "typedef struct fdcm_fit_params {" in header and "} fdcm_fit_params;" in header
    with open(os.path.join(root, "openfdcm_amd", "csrc", "fdcm_internal.h")) as f:
        assert "run_matches_fit" in f.read()
    with open(os.path.join(root, "README.md")) as f:
        readme = f.read()
    assert readme.index("## Match lists: refinement") < readme.index("## Match lists: pose fit") and "fit_matches" in readme
    with open(os.path.join(root, "DESIGN.md")) as f:
        assert "## 36. Match lists: pose fit" in f.read()
    with open(os.path.join(root, "INTEGRATION.md")) as f:
        assert "fdcm_matches_fit" in f.read()


def test_struct_sizes(capi):
    assert C.sizeof(capi.FitParams) == 32 and C.sizeof(capi.CoverageParams) == 12
    assert [(n, t) for n, t in capi.FitParams._fields_] == [("iterations", C.c_int32), ("min_pixels", C.c_int32), ("damping", C.c_double),
                                                            ("max_shift", C.c_double), ("max_angle", C.c_double)]
    assert [getattr(capi.FitParams, n).offset for n, _ in capi.FitParams._fields_] == [0, 4, 8, 16, 24]
    assert capi.MATCH_DTYPE.itemsize == 32


def test_python_signatures_and_defaults(capi):
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap
    p = inspect.signature(fd.fit_matches).parameters
    assert list(p) == ["featuremap", "labels", "templates", "matches", "radius", "bin_tolerance", "margin", "iterations", "min_pixels",
                       "damping", "max_shift", "max_angle", "return_info", "return_rms", "device_ptr", "n", "out_device_ptr"]
    assert p["radius"].default == 3 and p["bin_tolerance"].default == 1 and p["margin"].default is None and p["iterations"].default == 2
    assert p["min_pixels"].default == 8 and p["damping"].default == 1e-3 and p["max_shift"].default is None and p["max_angle"].default == 0.1
    assert p["return_info"].default is False and p["return_rms"].default is False and p["device_ptr"].default is None
    assert p["n"].default == 0 and p["out_device_ptr"].default is None
    assert "fit_matches" in dir(DeviceFeatureMap)
    # the siblings are as they were
    assert list(inspect.signature(fd.match_coverage).parameters) == ["featuremap", "labels", "templates", "matches", "radius", "bin_tolerance",
                                                                      "margin", "return_residual", "device_ptr", "n"]
    assert len({s[0]: s for s in capi.SYMBOLS}["fdcm_matches_coverage"][2]) == 13


def test_valid_arguments_reach_the_handles(capi):
    """The bounds are inclusive: with them the call goes on to the (null) handles."""
    for kw in [dict(), dict(n=0), dict(n=0, out=False), dict(matches=False, n=0, on_device=1), dict(matches=False, n=5), dict(on_device=1),
               dict(fit=(1, 3, 0.0, 0.0, 0.0)), dict(fit=(8, 1 << 30, 1e30, np.inf, np.inf)), dict(params=(0, 0, 0)),
               dict(params=(32, 1 << 20, 4096)), dict(width=1, height=1), dict(width=4096, height=4096), dict(out_on_device=1),
               dict(n=1 << 20)]:
        assert _fit(capi, **kw) == EINVAL and "null featuremap/templates" in _err(capi), kw


def test_every_refused_argument_is_einval_with_its_message(capi):
    # what fdcm_matches_coverage rejects
    assert _fit(capi, n=-1) == EINVAL and "n is negative" in _err(capi)
    assert _fit(capi, n=(1 << 20) + 1) == EINVAL and "n must be at most 2^20" in _err(capi)
    assert _fit(capi, on_device=2) == EINVAL and "on_device must be 0 or 1" in _err(capi)
    assert _fit(capi, matches=False, n=3, on_device=1) == EINVAL and "matches is null" in _err(capi)
    assert _fit(capi, params=None) == EINVAL and "params is null" in _err(capi)
    for r in (-1, 33):
        assert _fit(capi, params=(r, 1, 2)) == EINVAL and "radius must be in [0, 32]" in _err(capi)
    assert _fit(capi, params=(2, -1, 2)) == EINVAL and "bin_tolerance must be in [0, m / 2]" in _err(capi)
    for mg in (-1, 4097):
        assert _fit(capi, params=(2, 1, mg)) == EINVAL and "margin must be in [0, 4096]" in _err(capi)
    assert _fit(capi, labels=False) == EINVAL and "labels is null" in _err(capi)
    for w, h in [(0, 12), (16, 0), (4097, 12), (16, 4097), (-1, 12)]:
        assert _fit(capi, width=w, height=h) == EINVAL and "width and height must be in [1, 4096]" in _err(capi)
    # the call's own
    assert _fit(capi, fit=None) == EINVAL and "fit is null" in _err(capi)
    for v in (0, -1, 9):
        assert _fit(capi, fit=(v, 8, 1e-3, 3.0, 0.1)) == EINVAL and "iterations must be in [1, 8]" in _err(capi)
    for v in (2, 0, -5):
        assert _fit(capi, fit=(2, v, 1e-3, 3.0, 0.1)) == EINVAL and "min_pixels must be at least 3" in _err(capi)
    for v in (np.nan, -1e-9, -np.inf):
        assert _fit(capi, fit=(2, 8, v, 3.0, 0.1)) == EINVAL and "damping must be a number >= 0" in _err(capi)
        assert _fit(capi, fit=(2, 8, 1e-3, v, 0.1)) == EINVAL and "max_shift must be a number >= 0" in _err(capi)
        assert _fit(capi, fit=(2, 8, 1e-3, 3.0, v)) == EINVAL and "max_angle must be a number >= 0" in _err(capi)
    assert _fit(capi, out=False) == EINVAL and "out is null" in _err(capi)
    for v in (-1, 2):
        assert _fit(capi, out_on_device=v) == EINVAL and "out_on_device must be 0 or 1" in _err(capi)
    # in the order of the section: the list, the coverage parameters, the image, the fit, the outputs, then the handles
    assert _fit(capi, n=-1, params=None, fit=None) == EINVAL and "n is negative" in _err(capi)
    assert _fit(capi, params=None, labels=False, fit=None) == EINVAL and "params is null" in _err(capi)
    assert _fit(capi, labels=False, fit=None, out=False) == EINVAL and "labels is null" in _err(capi)
    assert _fit(capi, fit=(0, 0, -1.0, -1.0, -1.0), out=False) == EINVAL and "iterations" in _err(capi)
    assert _fit(capi, out=False, out_on_device=5) == EINVAL and "out is null" in _err(capi)


NO_DEVICE = """
import numpy as np
from openfdcm_amd import _capi
from openfdcm_amd.engine import DeviceFeatureMap
try:
    DeviceFeatureMap.build_labels(np.full((12, 16), 255, dtype=np.uint8), border=0, depth=6)
except _capi.FdcmError as e:
    print("refused:", e)
"""


def test_without_a_device_the_way_to_the_call_ends_in_ehip(capi):
    """fdcm_matches_fit needs a feature map and a template set, and both are made on a device: in a process that sees none the
    first of them fails with FDCM_EHIP (-2), so no caller reaches the call's GPU work.  With null handles the call itself is
    FDCM_EINVAL (above) and touches nothing."""
    root = os.path.abspath(os.path.join(os.path.dirname(capi.LIB_PATH), ".."))
    env = {**os.environ, "HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1", "PYTHONPATH": root}
    out = subprocess.run([sys.executable, "-c", NO_DEVICE], capture_output=True, text=True, timeout=120, env=env, cwd=root)
    assert out.returncode == 0 and "refused:" in out.stdout and "(code -2)" in out.stdout, out.stdout + out.stderr
