"""CPU-only checks of the hull footprints (include/fdcm.h, "Hull footprints"): the library exports the entry points and the
binding knows them, every argument check returns FDCM_EINVAL with a message before any handle or device is touched, and the
kind travels from with_footprint through the template cache to the handle's constructor.  What needs a handle (the kind's
getter on a real set, search() on a hull set) is in test_gpu_hull.py."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

EINVAL = -1
NEW_SYMBOLS = ["fdcm_templates_create_shaped", "fdcm_templates_footprint_kind", "fdcm_templates_footprint_spans",
               "fdcm_lines_footprint_spans"]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def i64(*v):
    return np.array(v, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))


def test_exports_and_binds_the_entry_points(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0] for s in capi.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in bound
    with open(os.path.join(os.path.dirname(capi.LIB_PATH), "..", "include", "fdcm.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert "int " + name + "(" in header
    assert "#define FDCM_FOOTPRINT_BOX 0" in header and "#define FDCM_FOOTPRINT_HULL 1" in header and "Hull footprints" in header
    assert (capi.FOOTPRINT_BOX, capi.FOOTPRINT_HULL) == (0, 1)
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceTemplates
    p = inspect.signature(DeviceTemplates.__init__).parameters
    assert p["footprint"].default == "box" and "line_caps" in p
    assert isinstance(DeviceTemplates.footprint, property) and callable(DeviceTemplates.footprint_spans)
    assert list(inspect.signature(DeviceTemplates.footprint_spans).parameters) == ["self", "cs", "pivots", "margin"]
    assert list(inspect.signature(fd.template_footprint_spans).parameters) == ["templates", "angles", "pivot", "margin"]
    assert list(inspect.signature(fd.with_footprint).parameters) == ["templates", "footprint"]


@pytest.mark.parametrize("kind", [-1, 2, 7, 1 << 30])
def test_a_kind_that_is_not_box_or_hull_is_einval(capi, kind):
    lines = np.zeros((2, 4), dtype=np.float32)
    h = C.c_void_p(1)
    rc = capi.lib().fdcm_templates_create_shaped(capi.fptr(lines), i64(0, 2), 1, None, kind, C.byref(h))
    assert rc == EINVAL and "footprint must be FDCM_FOOTPRINT_BOX or FDCM_FOOTPRINT_HULL" in _err(capi) and not h.value


def test_create_shaped_checks_what_create_capped_checks(capi):
    lines = np.zeros((2, 4), dtype=np.float32)
    caps = np.zeros(2, dtype=np.float32)
    h = C.c_void_p()
    f = capi.lib().fdcm_templates_create_shaped
    for kind in (0, 1):
        assert f(capi.fptr(lines), i64(0, 2), 1, capi.fptr(caps), kind, None) == EINVAL and "out is null" in _err(capi)
        assert f(capi.fptr(lines), None, 1, capi.fptr(caps), kind, C.byref(h)) == EINVAL and "bad offsets" in _err(capi)
        assert f(capi.fptr(lines), i64(0, 2), -1, capi.fptr(caps), kind, C.byref(h)) == EINVAL and "bad offsets" in _err(capi)
        assert f(capi.fptr(lines), i64(1, 2), 1, capi.fptr(caps), kind, C.byref(h)) == EINVAL and "offsets[0]" in _err(capi)
        assert f(capi.fptr(lines), i64(0, 2, 1), 2, capi.fptr(caps), kind, C.byref(h)) == EINVAL and "ascending" in _err(capi)
        bad = np.float32([0.0, np.nan])
        assert f(capi.fptr(lines), i64(0, 2), 1, capi.fptr(bad), kind, C.byref(h)) == EINVAL and "caps must be >= 0" in _err(capi)
    k = C.c_int32(5)
    assert capi.lib().fdcm_templates_footprint_kind(None, C.byref(k)) == EINVAL and "null" in _err(capi) and k.value == 5


def test_span_calls_check_their_arguments(capi):
    lines = np.zeros((2, 4), dtype=np.float32)
    off = np.zeros(4, dtype=np.int64)
    o = off.ctypes.data_as(C.POINTER(C.c_int64))
    f, g = capi.lib().fdcm_lines_footprint_spans, capi.lib().fdcm_templates_footprint_spans
    for margin in (-1, 4097, 1 << 30):
        assert f(capi.fptr(lines), i64(0, 2), 1, None, margin, o, None, None) == EINVAL and "margin must be in [0, 4096]" in _err(capi)
        assert g(None, None, margin, o, None, None) == EINVAL and "margin must be in [0, 4096]" in _err(capi)
    assert f(capi.fptr(lines), i64(0, 2), 1, None, 0, None, None, None) == EINVAL and "row_offsets is null" in _err(capi)
    assert g(None, None, 0, None, None, None) == EINVAL and "row_offsets is null" in _err(capi)
    assert g(None, None, 0, o, None, None) == EINVAL and "templates is null" in _err(capi)
    assert f(capi.fptr(lines), None, 2, None, 0, o, None, None) == EINVAL and "bad offsets" in _err(capi)
    assert f(capi.fptr(lines), i64(0, 1), -1, None, 0, o, None, None) == EINVAL and "bad offsets" in _err(capi)
    assert f(capi.fptr(lines), i64(1, 2), 1, None, 0, o, None, None) == EINVAL and "offsets[0] must be 0" in _err(capi)
    assert f(capi.fptr(lines), i64(0, 2, 1), 2, None, 0, o, None, None) == EINVAL and "ascending" in _err(capi)
    assert f(None, i64(0, 2), 1, None, 0, o, None, None) == EINVAL and "lines is null" in _err(capi)
    for cs, what in [(np.zeros((0, 2), dtype=np.float32), "n must be >= 1"), (np.float32([[1, 0], [np.nan, 0]]), "c and s must be finite")]:
        r = capi.Rotations(capi.fptr(cs), cs.shape[0], None)
        assert f(capi.fptr(lines), i64(0, 2), 1, C.byref(r), 0, o, None, None) == EINVAL and what in _err(capi)
        assert g(None, C.byref(r), 0, o, None, None) == EINVAL and what in _err(capi)
    cs, piv = np.float32([[1, 0]]), np.float32([[0, np.nan]])
    r = capi.Rotations(capi.fptr(cs), 1, capi.fptr(piv))
    assert f(capi.fptr(lines), i64(0, 2), 1, C.byref(r), 0, o, None, None) == EINVAL and "pivots must be finite" in _err(capi)
    # empty inputs: FDCM_OK and nothing but the first offset
    off[:] = 9
    assert f(None, None, 0, None, 0, o, None, None) == 0 and off[0] == 0 and (off[1:] == 9).all()
    assert f(capi.fptr(lines), i64(0, 0, 0), 2, None, 3, o, None, None) == 0 and (off[:3] == 0).all()  # templates without lines


def test_with_footprint_wraps_a_list_and_rejects_other_kinds():
    import openfdcm_amd as fd
    tm = [np.float32([[0, 0, 3, 4], [1, 1, 1, 6]]).T.copy(), np.zeros((4, 0), dtype=np.float32)]
    w = fd.with_footprint(tm, "hull")
    assert isinstance(w, list) and w.footprint == "hull" and len(w) == 2 and all(a is b for a, b in zip(w, tm))
    assert fd.with_footprint(tuple(tm), "box").footprint == "box"
    assert fd.with_footprint(w, "box").footprint == "box" and w.footprint == "hull"  # a new list: the old one keeps its kind
    for bad in ("Hull", "", "circle", None, 1, b"hull"):
        with pytest.raises(ValueError):
            fd.with_footprint(tm, bad)
    from openfdcm_amd.engine import footprint_kind
    assert (footprint_kind("box"), footprint_kind("hull")) == (0, 1)
    with pytest.raises(ValueError):
        footprint_kind("convex")


def test_the_kind_is_part_of_the_cache_key(monkeypatch):
    """The same arrays, plain and wrapped, get two handles; each is found again; a bad kind on a list raises."""
    import openfdcm_amd as fd
    made = []

    class Fake:
        def __init__(self, templates, line_caps=None, _packed=None, _caps=None, footprint="box"):
            self._h, self.kind, self.caps = 1, footprint, _caps
            made.append(self)

    monkeypatch.setattr(fd, "DeviceTemplates", Fake)
    cache = fd._TemplateCache()
    tm = [np.float32([[0, 0, 3, 4], [1, 1, 1, 6]]).T.copy(), np.float32([[2, 0, 2, 5]]).T.copy()]
    hull = fd.with_footprint(tm, "hull")
    a, b = cache.get(tm), cache.get(hull)
    assert (a.kind, b.kind) == ("box", "hull") and a is not b and len(made) == 2
    assert cache.get(tm) is a and cache.get(hull) is b and len(made) == 2
    c = cache.get(hull, line_caps=2.0)
    assert c.kind == "hull" and c.caps is not None and c is not b and cache.get(hull) is b and len(made) == 3
    box = fd.with_footprint(tm, "box")
    assert cache.get(box).kind == "box" and len(made) == 4  # another list object
    odd = fd.with_footprint(tm, "hull")
    odd.footprint = "disc"
    with pytest.raises(ValueError):
        cache.get(odd)
    assert len(made) == 4


def test_functions_that_take_templates_hand_the_list_on(monkeypatch):
    """Every public function with a `templates` argument gives the template cache the caller's own list, so a wrapped list
    keeps its kind: the two refined calls, which call other public functions, included."""
    import openfdcm_amd as fd
    seen = []

    class Stop(Exception):
        pass

    def get(templates, line_caps=None):
        seen.append(templates)
        raise Stop

    monkeypatch.setattr(fd._template_cache, "get", get)
    monkeypatch.setattr(fd, "_device_map", lambda fm: fm)
    tm = fd.with_footprint([np.float32([[0, 0, 3, 4], [1, 1, 1, 6]]).T.copy()], "hull")
    jobs = np.int32([[0, 0, 1, 0, 0, 1, 1]])
    calls = [
        lambda: fd.exhaustive_detect_nms(None, tm), lambda: fd.exhaustive_detect_all(None, tm, 1.0),
        lambda: fd.exhaustive_detect_objects(None, tm, [0], [1.0]), lambda: fd.exhaustive_detect_windows(None, tm, jobs, 1.0),
        lambda: fd.exhaustive_detect_windows_objects(None, tm, jobs, [0], [1.0]),
        lambda: fd.exhaustive_detect_refined(None, tm, 1.0, [0.0, 0.5], [0.0, 0.1], 2, 1, 2, 2),
        lambda: fd.exhaustive_detect_refined_objects(None, tm, [0], [1.0], [0.0, 0.5], [0.0, 0.1], 2, 1, 2, 2),
        lambda: fd.best_score_map(None, tm), lambda: fd.exhaustive_detect(None, tm, 2), lambda: fd.exhaustive_search(None, tm),
        lambda: fd.object_score_maps(None, tm, [0]),
    ]
    for call in calls:
        n = len(seen)
        with pytest.raises(Stop):
            call()
        assert len(seen) == n + 1 and seen[-1] is tm
    # the fine stage of the refined calls gets the same list as the coarse one
    got = {}
    for name in ("exhaustive_detect_all", "exhaustive_detect_objects", "exhaustive_detect_windows", "exhaustive_detect_windows_objects"):
        monkeypatch.setattr(fd, name, lambda fm, t, *a, _n=name, **k: got.setdefault(_n, t))
    monkeypatch.setattr(fd, "pose_windows", lambda *a, **k: np.zeros((0, 7), dtype=np.int32))
    fd.exhaustive_detect_refined(None, tm, 1.0, [0.0, 0.5], [0.0, 0.1], 2, 1, 2, 2)
    fd.exhaustive_detect_refined_objects(None, tm, [0], [1.0], [0.0, 0.5], [0.0, 0.1], 2, 1, 2, 2)
    assert set(got) == {"exhaustive_detect_all", "exhaustive_detect_objects", "exhaustive_detect_windows", "exhaustive_detect_windows_objects"}
    assert all(v is tm for v in got.values())
