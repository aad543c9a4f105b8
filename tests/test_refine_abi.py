"""Checks of fdcm_matches_refine (include/fdcm.h, "Match lists: refinement") that need no device: the library exports the entry
point, the binding and the header know it, the Python names have the stated signatures and defaults, delta_angles has its
exact zero, and every argument check returns FDCM_EINVAL with its own message before any handle or device is touched (the
handles are NULL throughout: a late check would report them instead).  The empty inputs need handles, which a process without a
device cannot make: they are in test_gpu_refine.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

EINVAL = -1
MATCH = np.dtype([("tmpl_idx", "<i4"), ("score", "<f4"), ("transform", "<f4", (6,))])
RECS = np.zeros(8, dtype=MATCH)
OUT = np.zeros(8, dtype=MATCH)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def _refine(capi, matches=True, n=8, on_device=0, cs=((1.0, 0.0), (0.5, 0.5), (0.0, 1.0)), pivots=None, rot_n=None, centre=0, hx=1, hy=1, sx=1,
            sy=1, out=True, out_on_device=0):
    rot = None
    if cs is not None:
        a = np.ascontiguousarray(cs, dtype=np.float32).reshape(-1, 2)
        rot = capi.Rotations(capi.fptr(a) if a.size else None, a.shape[0] if rot_n is None else rot_n, None)
        if pivots is not None:
            pv = np.ascontiguousarray(pivots, dtype=np.float32)
            rot.pivots = capi.fptr(pv)
    pose = np.zeros((8, 3), dtype=np.int32)
    return capi.lib().fdcm_matches_refine(None, None, C.c_void_p(RECS.ctypes.data) if matches else None, n, on_device, 0,
                                          C.byref(rot) if rot is not None else None, centre, hx, hy, sx, sy,
                                          C.c_void_p(OUT.ctypes.data) if out else None, out_on_device, pose.ctypes.data_as(C.POINTER(C.c_int32)))


def test_exports_declares_and_binds_the_entry_point(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0]: s for s in capi.SYMBOLS}
    root = os.path.join(os.path.dirname(capi.LIB_PATH), "..")
    with open(os.path.join(root, "include", "fdcm.h")) as f:
        header = f.read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    name = "fdcm_matches_refine"
    assert hasattr(lib, name) and name in bound and bound[name][1] is C.c_int and len(bound[name][2]) == 15
    decl = re.search(r"int %s\((.*?)\);" % name, plain, flags=re.S)
    assert decl and len(decl.group(1).split(",")) == 15
    names = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert names == ["fm", "templates", "matches", "n", "on_device", "tmpl_index_base", "rot", "centre", "hx", "hy", "sx", "sy", "out",
                     "out_on_device", "pose_out"]
    assert header.index("Match lists: scene coverage and selection") < header.index("Match lists: refinement") < header.index("host-side self checks")
    assert "tests/refine_ref.py" in header and "out.score is not s(out)" in header
    with open(os.path.join(root, "openfdcm_amd", "csrc", "fdcm_internal.h")) as f:
        internal = f.read()
    assert "run_matches_refine" in internal and "FDCM_REFINE_PART" in internal
    with open(os.path.join(root, "README.md")) as f:
        readme = f.read()
    assert readme.index("## Match lists: scene coverage and selection") < readme.index("## Match lists: refinement")
    assert "refine_matches" in readme and "delta_angles" in readme
    with open(os.path.join(root, "DESIGN.md")) as f:
        assert "## 35. Match lists: refinement" in f.read()
    with open(os.path.join(root, "INTEGRATION.md")) as f:
        assert "refine_matches" in f.read()


def test_python_signatures_and_defaults(capi):
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap
    p = inspect.signature(fd.refine_matches).parameters
    assert list(p) == ["featuremap", "templates", "matches", "angles", "pivot", "half_x", "half_y", "stride", "line_caps", "return_poses",
                       "device_ptr", "n", "out_device_ptr"]
    assert p["angles"].default is None and p["pivot"].default == "center" and p["half_x"].default == 0 and p["half_y"].default == 0
    assert p["stride"].default == 1 and p["line_caps"].default is None and p["return_poses"].default is False
    assert p["device_ptr"].default is None and p["n"].default == 0 and p["out_device_ptr"].default is None
    assert list(inspect.signature(fd.delta_angles).parameters) == ["half_steps", "step"]
    assert "refine_matches" in dir(DeviceFeatureMap)
    # the siblings are as they were
    assert list(inspect.signature(fd.verify_matches).parameters) == ["featuremap", "templates", "matches", "line_caps", "device_ptr", "n"]
    assert len({s[0]: s for s in capi.SYMBOLS}["fdcm_matches_verify"][2]) == 9


def test_delta_angles_has_its_exact_zero(capi):
    import openfdcm_amd as fd
    for half, step in ((0, 0.3), (1, np.deg2rad(1.0)), (5, np.deg2rad(1.0)), (7, 0.1), (3, -0.01)):
        a = fd.delta_angles(half, step)
        assert a.dtype == np.float64 and a.shape == (2 * half + 1,) and a[half] == 0.0
        assert np.array_equal(a, np.arange(-half, half + 1) * step)
        cs = fd._angles(a)
        assert cs.dtype == np.float32 and tuple(cs[half]) == (1.0, 0.0)
        assert [i for i in range(len(cs)) if tuple(cs[i]) == (1.0, 0.0)] == [half]


def test_valid_arguments_reach_the_handles(capi):
    """The bounds are inclusive: with them the call goes on to the (null) handles."""
    for kw in [dict(), dict(n=0), dict(n=0, out=False), dict(matches=False, n=0, on_device=1), dict(matches=False, n=5), dict(on_device=1),
               dict(cs=None, centre=0), dict(cs=None, centre=-1), dict(centre=-1), dict(centre=2), dict(hx=0, hy=0), dict(hx=4096, hy=0, cs=None),
               dict(hx=0, hy=4096, cs=None), dict(sx=4096, sy=4096), dict(out_on_device=1), dict(cs=[(1.0, 0.0)] * 65536, hx=0, hy=0),
               dict(cs=[(1.0, 0.0)] * 8, hx=15, hy=127, centre=7), dict(cs=[(2.0, 0.0), (0.0, 0.0)])]:
        assert _refine(capi, **kw) == EINVAL and "null featuremap/templates" in _err(capi), kw


def test_every_refused_argument_is_einval_with_its_message(capi):
    big = (1 << 22) + 1
    assert _refine(capi, n=-1) == EINVAL and "n is negative" in _err(capi)
    assert _refine(capi, n=big) == EINVAL and "n must be at most 2^22" in _err(capi)
    assert _refine(capi, matches=False, n=3, on_device=1) == EINVAL and "matches is null" in _err(capi)
    assert _refine(capi, on_device=2) == EINVAL and "on_device must be 0 or 1" in _err(capi)
    assert _refine(capi, rot_n=0) == EINVAL and "rotations: n must be >= 1" in _err(capi)
    assert _refine(capi, cs=np.zeros((0, 2)), rot_n=2) == EINVAL and "rotations: cs is null" in _err(capi)
    for bad in (np.nan, np.inf, -np.inf):
        assert _refine(capi, cs=[(1.0, 0.0), (bad, 0.0)]) == EINVAL and "rotations: c and s must be finite" in _err(capi)
        assert _refine(capi, cs=[(1.0, 0.0), (0.0, bad)]) == EINVAL and "rotations: c and s must be finite" in _err(capi)
    for v in (-2, 3, 1 << 20):
        assert _refine(capi, centre=v) == EINVAL and "centre must be in [-1, na - 1]" in _err(capi)
    for v in (1, 2):
        assert _refine(capi, cs=None, centre=v) == EINVAL and "centre must be in [-1, na - 1]" in _err(capi)
    for v in (-1, 4097):
        assert _refine(capi, hx=v) == EINVAL and "hx and hy must be in [0, 4096]" in _err(capi)
        assert _refine(capi, hy=v) == EINVAL and "hx and hy must be in [0, 4096]" in _err(capi)
    for v in (0, -1, 4097):
        assert _refine(capi, sx=v) == EINVAL and "sx and sy must be in [1, 4096]" in _err(capi)
        assert _refine(capi, sy=v) == EINVAL and "sx and sy must be in [1, 4096]" in _err(capi)
    for kw in (dict(cs=[(1.0, 0.0)] * 65537, hx=0, hy=0), dict(cs=[(1.0, 0.0)] * 8, hx=16, hy=128), dict(cs=None, hx=4096, hy=4),
               dict(cs=None, hx=4096, hy=4096)):
        assert _refine(capi, **kw) == EINVAL and "must be at most 65536" in _err(capi), kw
    assert _refine(capi, out=False) == EINVAL and "out is null" in _err(capi)
    for v in (-1, 2):
        assert _refine(capi, out_on_device=v) == EINVAL and "out_on_device must be 0 or 1" in _err(capi)
    # in the order of the section: the list, the table, the window, the outputs, then the handles
    assert _refine(capi, n=-1, centre=9, out=False) == EINVAL and "n is negative" in _err(capi)
    assert _refine(capi, rot_n=0, centre=9, hx=-1) == EINVAL and "rotations" in _err(capi)
    assert _refine(capi, centre=9, hx=-1, out=False) == EINVAL and "centre" in _err(capi)
    assert _refine(capi, hx=-1, sx=0, out=False) == EINVAL and "hx and hy" in _err(capi)
    assert _refine(capi, out=False, out_on_device=5) == EINVAL and "out is null" in _err(capi)
