"""GPU tests of the hull footprints (include/fdcm.h, "Hull footprints").  The referee is hull_ref.py: the shapes row by row in
integers and the greedy rule over them.  What the rule runs on comes from no code this feature touches:

  * fdcm_search_exhaustive_detect_nms has no threshold, so its referee runs on the planes of fdcm_best_map (held to
    detect_ref by test_gpu_detect.py) through hull_ref.hull_objects_nms;
  * every other call's candidates S_0 are the records of the same call on the BOX set at overlap_permille = cross_permille =
    1000, where nothing is suppressed: the whole of S_0 in key order, with boxes, fractions and jobs, held to the calls' own
    referees by the files that came with them.  hull_ref.hull_list_nms then applies the rule to the shapes of those entries,
    and the device's list on the HULL set must be those rows, byte for byte.

The case is tools/hull_probe.py's.  On it the referee alone gives different BOX and HULL lists wherever overlap < 1000 (a
build that silently used boxes fails), which is asserted before the device's list is looked at."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import hull_ref as hr
from detect_ref import records
from nms_ref import detect_nms_ref, footprints, point_boxes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tools", "hull_probe.py")
f32 = np.float32
CASES = [(True, (1, 1), 0), (True, (2, 3), 2), (False, (1, 1), 2)]  # rotations, strides, margin


def _load():
    spec = importlib.util.spec_from_file_location("hull_probe", PROBE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def probe():
    return _load()


class Rect:
    """The BOX footprint as a shape: every row of the box full."""

    def __init__(self, box):
        self.box = tuple(int(v) for v in box)
        n = max(0, self.box[3] - self.box[1] + 1)
        self.xl, self.xr = np.zeros(n, dtype=np.int64), np.full(n, self.box[2] - self.box[0], dtype=np.int64)
        self.area = n * (self.box[2] - self.box[0] + 1)


WORLDS = {}


def world(probe, case):
    if case in WORLDS:
        return WORLDS[case]
    from openfdcm_amd.engine import DeviceTemplates
    rot, stride, margin = case
    c = probe.case(rot, stride)
    c["margin"] = margin
    c["box"] = DeviceTemplates(c["tmpls"], line_caps=c["caps"])
    c["hull"] = DeviceTemplates(c["tmpls"], line_caps=c["caps"], footprint="hull")
    assert (c["box"].footprint, c["hull"].footprint) == ("box", "hull")
    c["A"] = 8 if rot else 1
    c["thr"], c["ms"] = probe.threshold(c, c["box"]), probe.object_thresholds(c, c["box"])
    c["shapes"] = hr.shapes(c["tmpls"], c["cs"], c["piv"], margin)
    c["boxes"] = footprints(c["tmpls"], c["cs"], c["piv"], margin)
    c["rects"] = [Rect(b) for b in c["boxes"].reshape(-1, 4)]
    assert [s.box for s in c["shapes"]] == [r.box for r in c["rects"]]
    x0, y0, nx, ny, sx, sy = c["grid"]
    if stride == (1, 1):
        assert nx > 16 and nx % 16 and ny > 64 and ny % 64, c["grid"]  # several sub-tiles, partial ones on both axes
    WORLDS[case] = c
    return c


def _bytes(parts):
    return [np.ascontiguousarray(p).tobytes() for p in parts]


def _rows(parts, idx):
    return [p[np.array(idx, dtype=np.int64)] for p in parts]


def _pair_and_translation(c, rec, box):
    t = int(rec["tmpl_idx"])
    a = 0
    if c["cs"] is not None:
        hit = np.flatnonzero((c["cs"][:, 0] == rec["transform"][0]) & (c["cs"][:, 1] == rec["transform"][3]))
        assert len(hit) == 1
        a = int(hit[0])
    b = c["boxes"][t, a]
    return t * c["A"] + a, (int(box[0]) - int(b[0]), int(box[1]) - int(b[1]))


def _entries(c, cand, kind):
    """The entries of hull_ref.hull_list_nms for the rows of a BOX list at overlap 1000: the list's order is the key order."""
    out = []
    for l in range(len(cand[0])):
        u, tr = _pair_and_translation(c, cand[0][l], cand[1][l])
        out.append((l, int(c["obj"][u // c["A"]]), c[kind][u], tr))
    return out


def _check_list(c, call, cross_of=lambda p: None, objects=False, name="", least=5):
    """call(tset, permille, cross, max_det) -> the call's outputs.  The candidates from the BOX set at 1000; the referee's BOX
    and HULL lists differ at 0 and 300; the device's HULL list is the referee's rows; at 1000 it is the candidates (identity 2);
    a list cut by max_detections is the leading part."""
    cand = call(c["box"], 1000, 1000, 4096)
    n = len(cand[0])
    assert 30 <= n < 4096, (name, n)
    assert _bytes(call(c["hull"], 1000, 1000, 4096)) == _bytes(cand)
    ent = {kind: _entries(c, cand, kind) for kind in ("shapes", "rects")}
    if not objects:
        ent = {k: [(key, 0, S, t) for key, o, S, t in v] for k, v in ent.items()}
    for permille in (0, 300):
        cross = cross_of(permille)
        want = hr.hull_list_nms(ent["shapes"], 4096, permille, cross)
        box = hr.hull_list_nms(ent["rects"], 4096, permille, cross)
        print(name, "permille", permille, "cross", cross, "candidates", n, "BOX list", len(box), "HULL list", len(want))
        assert want != box and len(want) >= least
        assert _bytes(call(c["box"], permille, cross, 4096)) == _bytes(_rows(cand, box))
        got = call(c["hull"], permille, cross, 4096)
        assert _bytes(got) == _bytes(_rows(cand, want))
        if permille == 300:
            assert _bytes(call(c["hull"], permille, cross, 4)) == _bytes(_rows(cand, want[:4]))
        if permille == 0 and cross in (None, 0):  # identity 4: no two returned shapes share a pixel; their boxes may
            px = [ent["shapes"][l][2].pixels(*ent["shapes"][l][3]) for l in want[:60]]
            assert all(not (px[i] & px[j]) for i in range(len(px)) for j in range(i))
            B = got[1][:60].astype(np.int64)
            meet = sum(1 for i in range(len(B)) for j in range(i)
                       if min(B[i, 2], B[j, 2]) >= max(B[i, 0], B[j, 0]) and min(B[i, 3], B[j, 3]) >= max(B[i, 1], B[j, 1]))
            print(name, "pairs of returned boxes that share a pixel:", meet)
            assert meet >= 1


@pytest.mark.parametrize("case", CASES)
def test_detect_nms(probe, case):
    c = world(probe, case)
    dev, grid = c["dev"], c["grid"]
    scores, pairs = dev.best_map(c["box"], grid, c["cs"], c["piv"], penalty=0)
    for permille in (0, 300, 1000):
        ent = hr.hull_objects_nms(scores, pairs, c["shapes"], grid, 64, permille)
        g = ent[:, 1]
        want = (records(g, scores.reshape(-1)[g], pairs, c["A"], c["cs"], c["piv"], grid), point_boxes(pairs, c["boxes"], grid)[g].astype(np.int32))
        box = detect_nms_ref(scores, pairs, c["boxes"].reshape(-1, 4), grid, 64, permille, c["A"], c["cs"], c["piv"])
        assert (_bytes(want) != _bytes(box)) == (permille < 1000)
        got = dev.exhaustive_detect_nms(c["hull"], grid, c["cs"], c["piv"], k=64, overlap_permille=permille, margin=c["margin"], penalty=0,
                                        boxes=True)
        assert 16 <= len(got[0]) == len(want[0]) <= 64 and _bytes(got) == _bytes(want)
        assert _bytes(dev.exhaustive_detect_nms(c["box"], grid, c["cs"], c["piv"], k=64, overlap_permille=permille, margin=c["margin"],
                                                penalty=0, boxes=True)) == _bytes(box)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("variant", ["all", "matched_winner", "matched_all"])
def test_detect_all(probe, case, variant):
    c = world(probe, case)
    mm = None if variant == "all" else 0.4
    gate = "all" if variant == "matched_all" else "winner"

    def call(tset, permille, cross, md):
        return c["dev"].exhaustive_detect_all(tset, c["grid"], c["cs"], c["piv"], max_score=c["thr"], max_detections=md,
                                              overlap_permille=permille, margin=c["margin"], penalty=0, boxes=True, min_matched=mm,
                                              matched=mm is not None, gate=gate)
    _check_list(c, call, name=variant)


def _ms(c):
    return c["ms"]


MM = np.array([0.0, 0.4, 0.2], dtype=np.float32)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("gate", ["winner", "all"])
def test_detect_objects(probe, case, gate):
    c = world(probe, case)

    def call(tset, permille, cross, md):
        return c["dev"].exhaustive_detect_objects(tset, c["grid"], c["obj"], _ms(c), probe.G, c["cs"], c["piv"], max_detections=md,
                                                  overlap_permille=permille, cross_permille=cross, margin=c["margin"], penalty=0,
                                                  min_matched=MM, boxes=True, matched=True, gate=gate)
    _check_list(c, call, cross_of=lambda p: {0: 200, 300: 100}[p], objects=True, name="objects " + gate)
    _check_list(c, call, cross_of=lambda p: p, objects=True, name="objects, cross = overlap, " + gate)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("variant", ["plain", "gated_all", "objects"])
def test_detect_windows(probe, case, variant):
    c = world(probe, case)
    sx, sy = c["stride"]

    def call(tset, permille, cross, md):
        if variant == "objects":
            return c["dev"].exhaustive_detect_windows_objects(tset, c["jobs"], c["obj"], _ms(c) * f32(2), probe.G, c["cs"], c["piv"], sx=sx,
                                                              sy=sy, wrap=True, max_detections=md, overlap_permille=permille,
                                                              cross_permille=cross, margin=c["margin"], penalty=0, min_matched=MM,
                                                              boxes=True, matched=True, job_index=True, gate="all")
        return c["dev"].exhaustive_detect_windows(tset, c["jobs"], c["cs"], c["piv"], sx=sx, sy=sy, wrap=True, max_detections=md, overlap_permille=permille, margin=c["margin"], penalty=0,
                                                  min_matched=0.4 if variant == "gated_all" else None, boxes=True, matched=True,
                                                  job_index=True, gate="all" if variant == "gated_all" else "winner")
    if variant == "objects":
        _check_list(c, call, cross_of=lambda p: {0: 200, 300: 100}[p], objects=True, name="windows objects")
    else:
        _check_list(c, call, name="windows " + variant)


def test_a_shape_taller_than_the_staged_rows(probe):
    """A two-line template of 1101 rows on a narrow, tall volume: the winner's spans are read from memory, not from LDS."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    keys, vol, tr = probe.volume(width=64, height=1300)
    dev = DeviceFeatureMap.from_volume(keys, vol, tr)
    tmpls = [np.float32([[2, 0, 30, 1100], [6, 0, 34, 1100]]).T.copy(), np.float32([[2, 0, 26, 1100], [7, 0, 31, 1100]]).T.copy()]
    c = dict(dev=dev, tmpls=tmpls, cs=None, piv=None, A=1, margin=1, obj=np.zeros(2, dtype=np.int32), stride=(1, 1))
    c["box"], c["hull"] = DeviceTemplates(tmpls), DeviceTemplates(tmpls, footprint="hull")
    c["grid"] = dev.exhaustive_window(c["box"], 1, 1).as_tuple()
    c["thr"] = probe.threshold(c, c["box"], 0.05)
    c["shapes"] = hr.shapes(tmpls, None, None, 1)
    c["boxes"] = footprints(tmpls, None, None, 1)
    c["rects"] = [Rect(b) for b in c["boxes"].reshape(-1, 4)]
    assert len(c["shapes"][0].xl) == 1103 and c["shapes"][0].area < c["rects"][0].area // 2

    def call(tset, permille, cross, md):
        return dev.exhaustive_detect_all(tset, c["grid"], max_score=c["thr"], max_detections=md, overlap_permille=permille, margin=1,
                                         penalty=0, boxes=True)
    cand = call(c["box"], 1000, 1000, 4096)
    assert (cand[0]["tmpl_idx"] == 0).sum() >= 5 and (cand[0]["tmpl_idx"] == 1).sum() >= 5
    _check_list(c, call, name="tall", least=2)


def test_identity_1_a_box_set_made_by_create_shaped_is_a_box_set(probe):
    from openfdcm_amd import _capi as capi
    from openfdcm_amd.engine import DeviceTemplates, flat_line_caps
    c = world(probe, CASES[1])
    flat, offsets = capi.pack_templates(c["tmpls"])
    caps = flat_line_caps(c["tmpls"], c["caps"], np.diff(offsets).tolist())
    shaped = DeviceTemplates(c["tmpls"], line_caps=c["caps"])
    capi.check(capi.lib().fdcm_templates_free(shaped._h))
    h = C.c_void_p()
    capi.check(capi.lib().fdcm_templates_create_shaped(capi.fptr(flat), offsets.ctypes.data_as(C.POINTER(C.c_int64)), len(c["tmpls"]),
                                                       capi.fptr(caps), 0, C.byref(h)))
    shaped._h = h
    assert shaped.footprint == "box"
    a, b = probe.calls(c, c["box"], c["thr"], c["ms"], c["margin"]), probe.calls(c, shaped, c["thr"], c["ms"], c["margin"])
    assert sorted(a) == sorted(b) and all(_bytes(a[k]) == _bytes(b[k]) and len(a[k][0]) >= 5 for k in a)
    # and the hull set's kind is what makes the difference, every call of the probe
    d = probe.calls(c, c["hull"], c["thr"], c["ms"], c["margin"])
    assert all(_bytes(a[k]) != _bytes(d[k]) for k in a), [k for k in a if _bytes(a[k]) == _bytes(d[k])]
    # identity 6: the same inputs, the same bytes
    e = probe.calls(c, c["hull"], c["thr"], c["ms"], c["margin"])
    assert all(_bytes(d[k]) == _bytes(e[k]) for k in d)
    # the shapes and boxes a handle reports do not depend on its kind
    for tset in (c["box"], c["hull"]):
        off, spans, areas = tset.footprint_spans(c["cs"], c["piv"], margin=c["margin"])
        want = hr.span_table(c["shapes"])
        assert np.array_equal(off, want[0]) and np.array_equal(spans, want[1]) and np.array_equal(areas, want[2])
        assert np.array_equal(tset.footprints(c["cs"], c["piv"], margin=c["margin"]), c["boxes"])


def test_identity_3_templates_that_hold_their_boxes_corners(probe):
    from openfdcm_amd.engine import DeviceTemplates
    c = dict(world(probe, CASES[2]))
    rng = np.random.default_rng(9)
    tmpls = []
    for t in range(5):
        x0, y0 = rng.uniform(-9, 9, size=2)
        w, h = rng.uniform(6, 30, size=2)
        tmpls.append(np.float32([[x0, y0, x0 + w, y0 + h], [x0 + w, y0, x0, y0 + h], [x0 + 1, y0 + 1, x0 + 2, y0 + 5]]).T.copy())
    quarter = np.array([[1, 0], [0, 1], [-1, 0], [0, -1]], dtype=np.float32)
    box, hull = DeviceTemplates(tmpls), DeviceTemplates(tmpls, footprint="hull")
    for cs in (None, quarter):
        grid = (c["dev"].exhaustive_window(box, 1, 1) if cs is None else c["dev"].exhaustive_rotations_window(box, cs, None, 1, 1)).as_tuple()
        for margin in (0, 2):
            for permille in (0, 300):
                a, b = (c["dev"].exhaustive_detect_all(s, grid, cs, None, max_score=float("inf"), max_detections=64,
                                                       overlap_permille=permille, margin=margin, penalty=0, boxes=True) for s in (box, hull))
                assert len(a[0]) >= 3 and _bytes(a) == _bytes(b)


def test_identity_5_and_7_on_a_hull_set(probe):
    c = world(probe, CASES[1])
    dev, grid, cs, piv = c["dev"], c["grid"], c["cs"], c["piv"]
    x0, y0, nx, ny, sx, sy = grid
    ms = _ms(c)
    kw = dict(max_detections=4096, margin=c["margin"], penalty=0, boxes=True, matched=True, gate="all")
    # identity 5: one-point jobs for every keyed entry of the object best map, by ascending (g, u)
    s, p = dev.best_map_objects(c["hull"], grid, c["obj"], probe.G, cs, piv, penalty=0, min_matched=MM)
    o, g = np.nonzero(p.reshape(probe.G, -1) >= 0)
    u = p.reshape(probe.G, -1)[o, g].astype(np.int64)
    order = np.lexsort((u, g))
    g, u = g[order], u[order]
    jobs = np.stack([u // 8, u % 8, np.ones_like(u), x0 + (g % nx) * sx, y0 + (g // nx) * sy, np.ones_like(u), np.ones_like(u)], axis=1).astype(np.int32)
    for permille, cross in [(300, 100), (0, 0)]:
        dense = dev.exhaustive_detect_objects(c["hull"], grid, c["obj"], ms, probe.G, cs, piv, overlap_permille=permille, cross_permille=cross,
                                              min_matched=MM, **kw)
        win = dev.exhaustive_detect_windows_objects(c["hull"], jobs, c["obj"], ms, probe.G, cs, piv, sx=sx, sy=sy, wrap=True,
                                                    overlap_permille=permille, cross_permille=cross, min_matched=MM, job_index=True, **kw)
        assert len(dense[0]) >= 10 and _bytes(win[:3]) == _bytes(dense)
    # identity 7: one object is the calls without objects
    one = np.zeros(len(c["tmpls"]), dtype=np.int32)
    for permille in (0, 300):
        old = dev.exhaustive_detect_all(c["hull"], grid, cs, piv, max_score=c["thr"], overlap_permille=permille, min_matched=0.4, **kw)
        new = dev.exhaustive_detect_objects(c["hull"], grid, one, c["thr"], 1, cs, piv, overlap_permille=permille, cross_permille=1000 - permille,
                                            min_matched=0.4, **kw)
        assert len(old[0]) >= 5 and _bytes(old) == _bytes(new)
        old = dev.exhaustive_detect_windows(c["hull"], c["jobs"], cs, piv, sx=sx, sy=sy, wrap=True, overlap_permille=permille,
                                            min_matched=0.4, job_index=True, **kw)
        new = dev.exhaustive_detect_windows_objects(c["hull"], c["jobs"], one, float("inf"), 1, cs, piv, sx=sx, sy=sy, wrap=True,
                                                    overlap_permille=permille, cross_permille=1000 - permille, min_matched=0.4, job_index=True,
                                                    **kw)
        assert len(old[0]) >= 5 and _bytes(old) == _bytes(new)


def test_the_public_functions_carry_the_kind(probe):
    """with_footprint through the template cache: the module-level calls on a wrapped list give the hull handle's bytes, and
    search() and the calls without an overlap treat a hull set as a box set."""
    import openfdcm_amd as fd
    c = world(probe, CASES[2])
    dev, grid = c["dev"], c["grid"]
    wrapped = fd.with_footprint(c["tmpls"], "hull")
    kw = dict(overlap=0.3, stride=1, penalty=fd.DefaultPenalty(), line_caps=c["caps"], margin=c["margin"], return_boxes=True)
    got = fd.exhaustive_detect_all(dev, wrapped, c["thr"], max_detections=4096, **kw)
    plain = fd.exhaustive_detect_all(dev, c["tmpls"], c["thr"], max_detections=4096, **kw)
    want = [dev.exhaustive_detect_all(s, grid, max_score=c["thr"], max_detections=4096, overlap_permille=300, margin=c["margin"], penalty=0,
                                      boxes=True) for s in (c["hull"], c["box"])]
    assert _bytes((got[0].records(), got[1])) == _bytes(want[0]) and _bytes((plain[0].records(), plain[1])) == _bytes(want[1])
    assert _bytes(want[0]) != _bytes(want[1])
    got = fd.exhaustive_detect_nms(dev, wrapped, k=16, **kw)
    want = dev.exhaustive_detect_nms(c["hull"], grid, k=16, overlap_permille=300, margin=c["margin"], penalty=0, boxes=True)
    assert _bytes((got[0].records(), got[1])) == _bytes(want)
    odd = fd.with_footprint(c["tmpls"], "hull")
    odd.footprint = "disc"
    with pytest.raises(ValueError):
        fd.exhaustive_detect_all(dev, odd, c["thr"])
    # calls without an overlap: the same bytes from both sets
    assert _bytes(dev.best_map(c["box"], grid, penalty=0)) == _bytes(dev.best_map(c["hull"], grid, penalty=0))
    assert dev.exhaustive_detect(c["box"], grid, k=8, rx=3, ry=3, penalty=0).tobytes() == \
        dev.exhaustive_detect(c["hull"], grid, k=8, rx=3, ry=3, penalty=0).tobytes()
    assert [x.tobytes() for x in c["hull"].line_caps()] == [x.tobytes() for x in c["box"].line_caps()]
    assert c["hull"].lengths().tobytes() == c["box"].lengths().tobytes()
    # search(), the reference's path: a wrapped list is the plain list
    scene = np.float32([[10, 10, 60, 40], [20, 80, 70, 30], [5, 50, 50, 120], [30, 20, 30, 90]]).T.copy()
    dt3 = fd.Dt3Cpu(None, _device=dev)
    a, b = (fd.records_of(fd.search(fd.DefaultMatch(), fd.DefaultSearch(4, 4), fd.BatchOptimize(4), dt3, t, scene)) for t in (c["tmpls"], wrapped))
    assert len(a) > 0 and a.tobytes() == b.tobytes()


def test_a_span_table_of_more_than_2_26_rows_is_einval(probe):
    """Three templates whose boxes are 2^25 rows high: the dense calls on the hull set refuse before any device work; the box
    set, the calls without an overlap and the offsets of the span call do not mind."""
    from openfdcm_amd._capi import FdcmError
    from openfdcm_amd.engine import DeviceTemplates
    c = world(probe, CASES[2])
    dev = c["dev"]
    tall = [np.float32([[0, 0, 3, 4e7]]).T.copy() for _ in range(3)]
    box, hull = DeviceTemplates(tall), DeviceTemplates(tall, footprint="hull")
    grid = (0, 0, 4, 4, 1, 1)
    obj = np.zeros(3, dtype=np.int32)
    for call in (lambda s: dev.exhaustive_detect_nms(s, grid, k=4), lambda s: dev.exhaustive_detect_all(s, grid, max_detections=4),
                 lambda s: dev.exhaustive_detect_all(s, grid, max_detections=4, min_matched=0.5, gate="all"),
                 lambda s: dev.exhaustive_detect_objects(s, grid, obj, float("inf"), 1, max_detections=4)):
        assert len(call(box)) == 0  # no admissible point: an empty list
        with pytest.raises(FdcmError, match="2\\^26 rows"):
            call(hull)
    assert len(dev.exhaustive_detect(hull, grid, k=4)) == 0 and np.isnan(dev.best_map(hull, grid)[0]).all()
    import openfdcm_amd as fd
    assert fd.template_footprints(tall)[0, 0].tolist() == [0, 0, 3, 1 << 25]
    two = DeviceTemplates(tall[:1], footprint="hull")  # 2^25 + 1 rows: within the limit
    assert len(dev.exhaustive_detect_all(two, grid, max_detections=4)) == 0


def test_the_rod_scene(probe):
    """Two parallel rods at 45 degrees, 14 px apart, one rod template and the 8-angle table: the BOX set finds one rod, the HULL
    set both, on the referee and on the device."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    from test_hull_definition import rod
    shift = np.float32([[140, 140, 140, 140]]).T  # rod() centres its rods at (200, 200)
    scene = np.concatenate([rod(60, 10, 45, 0), rod(60, 10, 45, 14)], axis=1) - shift
    tm = rod(60, 10, 0, 0) - np.float32([[200, 200, 200, 200]]).T
    dev = DeviceFeatureMap.build(scene, depth=12, coeff=5.0, padding=1.5, distance=0)
    cs = probe.cs_table()
    piv = np.zeros((1, 2), dtype=np.float32)
    box, hull = DeviceTemplates([tm]), DeviceTemplates([tm], footprint="hull")
    grid = dev.exhaustive_rotations_window(box, cs, piv, 1, 1).as_tuple()
    s = dev.best_map(box, grid, cs, piv, penalty=0)[0]
    thr = float(np.nanmin(s)) * 2.5 + 0.5
    print("rod scene: grid", grid, "best score", float(np.nanmin(s)), "threshold", thr, "points under it", int((s <= thr).sum()))
    c = dict(cs=cs, A=8, obj=np.zeros(1, dtype=np.int32), boxes=footprints([tm], cs, piv, 0), shapes=hr.shapes([tm], cs, piv, 0))
    c["rects"] = [Rect(b) for b in c["boxes"].reshape(-1, 4)]

    def call(tset, permille):
        return dev.exhaustive_detect_all(tset, grid, cs, piv, max_score=thr, max_detections=4096, overlap_permille=permille, margin=0,
                                         penalty=0, boxes=True)
    cand = call(box, 1000)
    assert 2 <= len(cand[0]) < 4096
    ref = {kind: hr.hull_list_nms([(k, 0, S, t) for k, o, S, t in _entries(c, cand, kind)], 4096, 300) for kind in ("rects", "shapes")}
    print("rod scene: candidates", len(cand[0]), "referee BOX", len(ref["rects"]), "HULL", len(ref["shapes"]))
    assert len(ref["rects"]) == 1 and len(ref["shapes"]) == 2
    got = {"rects": call(box, 300), "shapes": call(hull, 300)}
    for kind in ref:
        assert _bytes(got[kind]) == _bytes(_rows(cand, ref[kind]))
    # the two detections are the two rods: both at 45 (or 225) degrees, 14 px apart along the normal
    t = got["shapes"][0]["transform"]
    assert all(abs(abs(float(v[0])) - np.sqrt(0.5)) < 1e-6 for v in t)


def test_poison_does_not_matter(probe):
    """The hull dense and window calls in fresh processes with and without FDCM_POISON, each under its own time limit; the
    first process that differs or dies ends the test, and nothing more is started."""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}
    base = None
    for env in ({}, {"FDCM_POISON": "1"}, {"FDCM_POISON": "0xffffffff"}):
        out = subprocess.run([sys.executable, PROBE], capture_output=True, text=True, timeout=240, env={**clean, **env})
        assert out.returncode == 0, (env, out.stdout[-2000:] + out.stderr[-4000:])
        lines = sorted(l for l in out.stdout.splitlines() if l.startswith("hull_probe "))
        assert len(lines) == 16 and all(int(l.split()[3]) >= 5 for l in lines), lines
        if base is None:
            base = lines
        assert lines == base, (env, [a for a, b in zip(lines, base) if a != b])
