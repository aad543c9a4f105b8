"""CPU-only checks of the image pyramid (include/fdcm.h, "image pyramid"): the entry points are exported as declared, the size
recurrence, every argument error is FDCM_EINVAL with a message that names the argument before any device work, the Python
signatures, scaled_templates / lift_records on bit patterns, the lift identity in numpy float32, and the driver's job arrays
against the written-out composition with the two device calls replaced by recorders.  No call here reaches a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import pyramid_ref as R
from helpers import ROOT

EINVAL = -1
NEW_SYMBOLS = {"fdcm_image_pyramid_size": 5, "fdcm_image_pyramid_level": 8, "fdcm_featuremap_build_image_level": 12,
               "fdcm_featuremap_rebuild_image_level": 9}


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_exports_the_pyramid_entry_points_as_declared(capi):
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
            elif p.startswith("int32_t"):
                assert ct is C.c_int32, (name, p, ct)
            elif p.startswith("float"):
                assert ct is C.c_float, (name, p, ct)
            else:
                assert p.startswith("int ") and ct is C.c_int, (name, p, ct)


# ---------------------------------------------------------------- sizes
@pytest.mark.parametrize("level", [0, 1, 11, 12])
@pytest.mark.parametrize("size", [1, 2, 3, 4095, 4096])
def test_pyramid_size_is_the_recurrence(capi, size, level):
    from openfdcm_amd import image_pyramid_size
    for width, height in ((size, size), (size, 7), (5, size)):
        w, h = C.c_int64(-1), C.c_int64(-1)
        assert capi.lib().fdcm_image_pyramid_size(width, height, level, C.byref(w), C.byref(h)) == 0
        assert (w.value, h.value) == R.level_size(width, height, level) == image_pyramid_size(width, height, level)
    # the recurrence, written out once more: a ceiling division by 2^level, never below 1
    assert R.level_size(size, size, level)[0] == max(1, -(-size >> level))


@pytest.mark.parametrize("args,what", [((10, 8, -1), "level"), ((10, 8, 13), "level"), ((0, 8, 1), "width and height"),
                                       ((10, 0, 1), "width and height"), ((4097, 8, 1), "4096"), ((10, 4097, 0), "4096"),
                                       ((-3, 8, 0), "width and height")], ids=str)
def test_pyramid_size_argument_errors(capi, args, what):
    w, h = C.c_int64(-7), C.c_int64(-7)
    assert capi.lib().fdcm_image_pyramid_size(*args, C.byref(w), C.byref(h)) == EINVAL
    assert what in _err(capi), _err(capi)
    assert (w.value, h.value) == (-7, -7)
    assert capi.lib().fdcm_image_pyramid_size(10, 8, 1, None, C.byref(h)) == EINVAL and "w_out is null" in _err(capi)
    assert capi.lib().fdcm_image_pyramid_size(10, 8, 1, C.byref(w), None) == EINVAL and "h_out is null" in _err(capi)
    assert (w.value, h.value) == (-7, -7)


# ---------------------------------------------------------------- argument errors of the calls that would reach a device
IMG = np.zeros((8, 10), dtype=np.uint8)
GOOD = dict(smooth=1, low=20, high=60, min_pixels=8)


def _params(capi, kw):
    if kw.get("params", True) is None:
        return None
    v = dict(GOOD, **{k: kw[k] for k in GOOD if k in kw})
    return C.byref(capi.EdgeParams(v["smooth"], v["low"], v["high"], v["min_pixels"]))


def _build(capi, image=IMG, width=10, height=8, stride=10, on_device=0, level=1, border=0, depth=6, distance=0, out=True, **kw):
    h = C.c_void_p(0xdead)
    p = C.c_void_p(image.ctypes.data) if image is not None else None
    rc = capi.lib().fdcm_featuremap_build_image_level(p, width, height, stride, on_device, level, _params(capi, kw), border, depth, 5.0,
                                                      distance, C.byref(h) if out else None)
    if out and rc != 0:
        assert h.value is None          # a failed build hands out no handle
    return rc


LEVEL_ERRORS = [
    (dict(level=-1), "level"), (dict(level=13), "level"), (dict(level=1 << 20), "level"),
    (dict(width=4097, stride=4097), "4096"), (dict(height=4097), "4096"), (dict(width=4097, stride=4097, level=12), "4096"),
    (dict(width=4096, stride=4096, level=0, border=1), "4096"), (dict(width=4096, stride=4096, level=1, border=1025), "4096"),
]
PARAM_ERRORS = [
    (dict(params=None), "params is null"),
    (dict(smooth=-1), "smooth"), (dict(smooth=3), "smooth"),
    (dict(low=0), "low"), (dict(high=1443), "high"), (dict(low=61), "low"),
    (dict(min_pixels=0), "min_pixels"),
]
SIBLING_ERRORS = [
    (dict(image=None), "image is null"),
    (dict(out=False), "out is null"),
    (dict(border=-1), "border"),
    (dict(width=0), "width and height"), (dict(height=0), "width and height"), (dict(width=-4), "width and height"),
    (dict(stride=9), "row_stride"),
    (dict(depth=256), "255"), (dict(depth=-1), "depth"),
    (dict(distance=3), "distance"),
    (dict(on_device=2), "on_device"),
]


@pytest.mark.parametrize("kw,what", LEVEL_ERRORS + PARAM_ERRORS + SIBLING_ERRORS, ids=lambda v: str(v))
def test_build_image_level_argument_errors(capi, kw, what):
    assert _build(capi, **kw) == EINVAL
    assert what in _err(capi), _err(capi)


def test_rebuild_image_level_without_a_handle(capi):
    """(The handle is checked first; a rebuild's other errors need a handle, so tests/test_gpu_pyramid.py has them.)"""
    p = C.c_void_p(IMG.ctypes.data)
    assert capi.lib().fdcm_featuremap_rebuild_image_level(None, p, 10, 8, 10, 0, 1, _params(capi, {}), 0) == EINVAL
    assert "featuremap is null" in _err(capi)


def _level(capi, image=IMG, width=10, height=8, stride=10, on_device=0, level=1, out=True, out_on_device=0):
    buf = np.full(80, 0xA5, dtype=np.uint8)
    p = C.c_void_p(image.ctypes.data) if image is not None else None
    rc = capi.lib().fdcm_image_pyramid_level(p, width, height, stride, on_device, level, C.c_void_p(buf.ctypes.data) if out else None,
                                             out_on_device)
    assert (buf == 0xA5).all()          # a refused call writes nothing
    return rc


@pytest.mark.parametrize("kw,what", [
    (dict(level=-1), "level"), (dict(level=13), "level"),
    (dict(image=None), "image is null"), (dict(out=False), "out is null"),
    (dict(width=0), "width and height"), (dict(height=0), "width and height"), (dict(height=-1), "width and height"),
    (dict(width=4097, stride=4097), "4096"), (dict(height=4097), "4096"), (dict(width=4097, stride=4097, level=0), "4096"),
    (dict(stride=9), "row_stride"), (dict(on_device=2), "on_device"), (dict(on_device=-1), "on_device"),
    (dict(out_on_device=2), "out_on_device")], ids=lambda v: str(v))
def test_image_pyramid_level_argument_errors(capi, kw, what):
    assert _level(capi, **kw) == EINVAL
    assert what in _err(capi), _err(capi)


# ---------------------------------------------------------------- Python layer
def _names(fn):
    return list(inspect.signature(fn).parameters)


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def test_python_signatures(capi):
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap
    assert _names(fd.image_pyramid) == ["image", "level"]
    assert _names(fd.scaled_templates) == ["templates", "level"]
    assert _names(fd.lift_records) == ["records", "level"]
    assert _names(fd.build_image_featuremap_level) == ["image", "level", "params", "threshold", "border", "low", "smooth", "min_pixels"]
    assert _defaults(fd.build_image_featuremap_level) == _defaults(fd.build_image_featuremap)
    assert _names(DeviceFeatureMap.build_image_level)[:3] == ["image", "level", "threshold"]
    assert _names(DeviceFeatureMap.rebuild_image_level)[:4] == ["self", "image", "level", "threshold"]
    for fn in (DeviceFeatureMap.build_image_level, DeviceFeatureMap.rebuild_image_level):
        d = _defaults(fn)
        assert (d["border"], d["low"], d["smooth"], d["min_pixels"]) == (0, None, 0, 1), fn
    lead = ["featuremap", "level_featuremap", "level", "templates", "max_score", "coarse_angles", "fine_angles", "half_angles", "half_x",
            "half_y", "coarse_stride", "coarse_max_score", "coarse_overlap", "coarse_max_detections", "coarse_line_caps", "coarse_margin"]
    refined = _names(fd.exhaustive_detect_refined)
    assert _names(fd.exhaustive_detect_pyramid) == lead + refined[refined.index("overlap"):]
    d, dr = _defaults(fd.exhaustive_detect_pyramid), _defaults(fd.exhaustive_detect_refined)
    assert (d["half_x"], d["half_y"], d["coarse_stride"], d["coarse_line_caps"], d["coarse_margin"]) == (None, None, 1, None, None)
    assert all(d[k] == dr[k] for k in dr)
    lead_o = lead[:4] + ["objects"] + lead[4:13] + ["coarse_cross_overlap"] + lead[13:]
    refined_o = _names(fd.exhaustive_detect_refined_objects)
    assert _names(fd.exhaustive_detect_pyramid_objects) == lead_o + refined_o[refined_o.index("overlap"):]
    d, dr = _defaults(fd.exhaustive_detect_pyramid_objects), _defaults(fd.exhaustive_detect_refined_objects)
    assert all(d[k] == dr[k] for k in dr)
    img = np.zeros((8, 10), dtype=np.uint8)
    for level in (-1, 13):
        with pytest.raises(fd._capi.FdcmError, match="level"):
            fd.image_pyramid(img, level)
        with pytest.raises(fd._capi.FdcmError, match="level"):
            DeviceFeatureMap.build_image_level(img, level, 60, depth=6)
        with pytest.raises(ValueError, match="level"):
            fd.scaled_templates([np.zeros((4, 1), dtype=np.float32)], level)
        with pytest.raises(ValueError, match="level"):
            fd.lift_records(np.zeros(0, dtype=fd._capi.MATCH_DTYPE), level)
    with pytest.raises(ValueError):
        fd.image_pyramid(np.zeros((4, 4), dtype=np.float32), 1)


def _templates(rng, n=5):
    out = [rng.uniform(-300, 300, size=(4, int(k))).astype(np.float32) for k in rng.integers(1, 9, size=n)]
    out[0][:, 0] = (-0.0, 0.0, -1.5, 3.0)                       # a negative zero and a positive one
    out.append(np.zeros((4, 0), dtype=np.float32))              # a template without lines
    return out


@pytest.mark.parametrize("level", [0, 1, 2, 5, 12])
def test_scaled_templates_and_lift_records_are_ldexp(capi, level):
    import openfdcm_amd as fd
    rng = np.random.default_rng(level)
    tm = _templates(rng)
    small = fd.scaled_templates(tm, level)
    assert type(small) is list and len(small) == len(tm)
    for a, b in zip(tm, small):
        assert b.dtype == np.float32 and b.shape == a.shape
        assert np.array_equal(bits(b), bits(np.ldexp(a, -level)))
    assert bits(small[0][0, 0]) == 0x80000000 and bits(small[0][1, 0]) == 0            # -0 stays -0
    assert small[-1].shape == (4, 0)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(tm, _templates(np.random.default_rng(level))))  # input untouched
    # float64 input is taken as the library takes it: rounded to float32 first
    assert np.array_equal(bits(fd.scaled_templates([tm[1].astype(np.float64)], level)[0]), bits(small[1]))
    for kind in ("box", "hull"):
        shaped = fd.scaled_templates(fd.with_footprint(tm, kind), level)
        assert isinstance(shaped, list) and shaped.footprint == kind
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(shaped, small))
    assert not hasattr(small, "footprint")
    dt = object.__new__(fd.DeviceTemplates)                      # (no handle: the type alone is refused)
    dt._h = None
    with pytest.raises(ValueError, match="DeviceTemplates"):
        fd.scaled_templates(dt, level)

    rec = np.zeros(6, dtype=fd._capi.MATCH_DTYPE)
    rec["tmpl_idx"] = rng.integers(0, 5, size=6)
    rec["score"] = rng.uniform(0, 3, size=6).astype(np.float32)
    rec["transform"] = rng.uniform(-2000, 2000, size=(6, 6)).astype(np.float32)
    rec["transform"][0, 2] = -0.0
    before = rec.copy()
    up = fd.lift_records(rec, level)
    assert isinstance(up, np.ndarray) and up.dtype == rec.dtype and up is not rec and rec.tobytes() == before.tobytes()
    want = before.copy()
    want["transform"][:, 2] = np.ldexp(before["transform"][:, 2], level)
    want["transform"][:, 5] = np.ldexp(before["transform"][:, 5], level)
    assert up.tobytes() == want.tobytes()
    assert bits(up["transform"][0, 2]) == 0x80000000
    ml = fd.lift_records(fd.MatchList(before.copy()), level)
    assert isinstance(ml, fd.MatchList) and ml.records().tobytes() == want.tobytes()
    assert len(fd.lift_records(np.zeros(0, dtype=rec.dtype), level)) == 0


# ---------------------------------------------------------------- the lift identity
@pytest.mark.parametrize("level", [1, 2, 3, 7, 12])
@pytest.mark.parametrize("pivot", ["center", "explicit", None])
def test_lifted_record_is_the_level0_record(capi, level, pivot):
    """For random templates, pivots, angle tables and integer t_L: the level-L record, built by the documented float32 rule
    from the scaled pivot, lifts to the level-0 record of 2^L t_L bit for bit, and pose_windows reads (tmpl, a, 2^L t_L)."""
    import openfdcm_amd as fd
    rng = np.random.default_rng(100 * level + len(str(pivot)))
    tm = _templates(rng, 6)
    T = len(tm)
    pv = None if pivot is None else (fd.template_pivots(tm, "center") if pivot == "center" else
                                     rng.uniform(-500, 500, size=(T, 2)).astype(np.float32))
    small = fd.scaled_templates(tm, level)
    if pivot == "center":   # the scaled list's own centres are the scaled centres
        assert np.array_equal(bits(fd.template_pivots(small, "center")), bits(np.ldexp(pv, -level)))
    angles = np.sort(rng.uniform(0, 2 * np.pi, size=23))
    cs = fd._angles(angles)
    # (a table with two equal rotations would make "the" index ambiguous)
    assert len({(c.tobytes(), s.tobytes()) for c, s in cs}) == len(cs)
    n = 64
    rec_l = np.zeros(n, dtype=fd._capi.MATCH_DTYPE)
    rec_0 = np.zeros(n, dtype=fd._capi.MATCH_DTYPE)
    want = np.zeros((n, 7), dtype=np.int32)
    span = 4096 >> level
    for q in range(n):
        t, a = int(rng.integers(0, T)), int(rng.integers(0, len(angles)))
        tl = rng.integers(-span, span + 1, size=2)
        p0 = np.zeros(2, dtype=np.float32) if pv is None else pv[t]
        pl = p0 * np.float32(2.0 ** -level)
        rec_l[q] = (t, rng.uniform(0, 2), R.record_transform(cs[a, 0], cs[a, 1], pl, tl))
        rec_0[q] = (t, rec_l[q]["score"], R.record_transform(cs[a, 0], cs[a, 1], p0, tl * 2 ** level))
        want[q] = (t, a, 1, tl[0] * 2 ** level, tl[1] * 2 ** level, 1, 1)
    up = fd.lift_records(rec_l, level)
    assert up.tobytes() == rec_0.tobytes()
    jobs = fd.pose_windows(up, angles, angles, pv, 0, 0, 0)
    assert np.array_equal(jobs, want)


# ---------------------------------------------------------------- the driver is its composition (device calls recorded)
@pytest.mark.parametrize("with_objects", [False, True])
@pytest.mark.parametrize("level,pivot,margin,coarse_margin,half", [(1, "center", 0, None, None), (2, None, 5, None, (3, 1)),
                                                                     (3, "explicit", 9, 2, None)])
def test_driver_builds_the_written_out_jobs(capi, monkeypatch, with_objects, level, pivot, margin, coarse_margin, half):
    import openfdcm_amd as fd
    rng = np.random.default_rng(7 * level)
    tm = fd.with_footprint(_templates(rng, 4), "hull") if level == 2 else _templates(rng, 4)
    T = len(tm)
    pivot = rng.uniform(-50, 50, size=(T, 2)).astype(np.float32) if pivot == "explicit" else pivot
    pv = fd.template_pivots(tm, pivot)
    coarse, fine = np.deg2rad(np.arange(0, 360, 30.0)), np.deg2rad(np.arange(0, 360, 2.0))
    cs = fd._angles(coarse)
    seeds_l = np.zeros(9, dtype=fd._capi.MATCH_DTYPE)
    for q in range(len(seeds_l)):
        t, a = q % (T - 1), (5 * q) % len(coarse)
        pl = np.zeros(2, dtype=np.float32) if pv is None else pv[t] * np.float32(2.0 ** -level)
        seeds_l[q] = (t, 0.1 * q, R.record_transform(cs[a, 0], cs[a, 1], pl, rng.integers(0, 200, size=2)))
    seen = {}

    def coarse_call(fm, templates, *args, **kw):
        seen["coarse"] = (fm, templates, args, kw)
        return fd.MatchList(seeds_l.copy())

    def fine_call(fm, templates, jobs, *args, **kw):
        seen["fine"] = (fm, templates, jobs, args, kw)
        return "fine result"

    objects = np.arange(T) % 2
    if with_objects:
        monkeypatch.setattr(fd, "exhaustive_detect_objects", coarse_call)
        monkeypatch.setattr(fd, "exhaustive_detect_windows_objects", fine_call)
        lead, driver = (tm, objects, 0.7), fd.exhaustive_detect_pyramid_objects
    else:
        monkeypatch.setattr(fd, "exhaustive_detect_all", coarse_call)
        monkeypatch.setattr(fd, "exhaustive_detect_windows", fine_call)
        lead, driver = (tm, 0.7), fd.exhaustive_detect_pyramid
    kw = dict(coarse_max_score=None if level == 1 else 2.5, coarse_margin=coarse_margin, margin=margin, pivot=pivot, wrap=level == 2,
              stride=2 if level == 3 else 1, coarse_line_caps=1.5, line_caps=3.0, gate="all", min_matched=0.5)
    if half is not None:
        kw.update(half_x=half[0], half_y=half[1])
    assert driver("map0", "mapL", level, *lead, coarse, fine, 4, **kw) == "fine result"

    hx, hy = half if half is not None else (2 ** level, 2 ** level)
    jobs = fd.pose_windows(fd.lift_records(seeds_l, level), coarse, fine, pv, 4, hx, hy, stride=kw["stride"], wrap=kw["wrap"])
    fm, templates, got_jobs, args, fkw = seen["fine"]
    assert fm == "map0" and templates is tm and np.array_equal(got_jobs, jobs) and got_jobs.dtype == np.int32
    assert args[-1] == 0.7 and fkw["angles"] is fine and fkw["line_caps"] == 3.0 and fkw["margin"] == margin and fkw["gate"] == "all"
    assert fkw["pivot"] is pivot and fkw["min_matched"] == 0.5 and fkw["wrap"] == kw["wrap"] and fkw["stride"] == kw["stride"]
    fm, templates, args, ckw = seen["coarse"]
    assert fm == "mapL" and getattr(templates, "footprint", None) == getattr(tm, "footprint", None)
    assert all(np.array_equal(bits(a), bits(np.ldexp(np.asarray(b), -level))) for a, b in zip(templates, tm))
    assert args[-1] == (float("inf") if level == 1 else 2.5)
    assert ckw["margin"] == (coarse_margin if coarse_margin is not None else -(-margin // 2 ** level))
    assert ckw["line_caps"] == 1.5 and ckw["stride"] == 1 and ckw["angles"] is coarse and ckw["overlap"] == 1.0
    assert "min_matched" not in ckw and "gate" not in ckw
    if pv is None:
        assert ckw["pivot"] is None
    else:
        assert np.array_equal(bits(ckw["pivot"]), bits(np.ldexp(pv, -level)))
    if with_objects:
        assert args[0] is objects and seen["fine"][3][0] is objects
