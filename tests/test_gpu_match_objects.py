"""GPU tests of the match lists with objects and hull shapes (include/fdcm.h, "Match lists: objects and hull shapes"):
fdcm_matches_detect_objects, fdcm_matches_shapes and fdcm_matches_footprint_spans equal the referee (tests/match_objects_ref.py:
match_ref, hull_ref and Python integers, nothing from the kernels) byte for byte -- there is no tolerance to choose.  The worlds
are test_gpu_matches.py's two maps (the line-built map of a 90-line scene at depth 12 and the adopted 70 x 37 x 6 volume with a
NaN and an infinity), templates of 0 to 130 lines, four kinds of caps and the 700 records of every kind match_cases.record_list
makes; objects are t % 3.

The shapes kernel: the device's span table equals the host's for every admissible record at margins 0, 1 and 3 (one line, 64,
65 and 130 lines, more than 1024 vertices at a margin), on horizontal, vertical and zero-length lines, collinear triples and
duplicate vertices, and on a shape of more than 1024 rows whose rows the round reads from memory.  Then detect against the
referee on box and hull sets, the rounds across a batch, the cases' own discrimination, the identities 1 to 7 and 9, the
switches and FDCM_POISON in fresh processes (tools/match_objects_probe.py), the refusals that need handles, and two scenes end
to end."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import hull_ref
import match_cases as MC
import match_objects_ref as MO
import match_ref as R
from helpers import ROOT
from test_gpu_matches import same_detection, world

pytestmark = pytest.mark.gpu
PROBE = os.path.join(ROOT, "tools", "match_objects_probe.py")
MAPS = ("lines", "adopted")
LIMITS = ((300, 300, 0), (300, 800, 0), (150, 1000, 3), (0, 0, 0), (1000, 1000, 0))   # (permille, cross, margin)
MS, MM = [30.0, 18.0, 35.0], [0.0, 0.3, 0.6]


def objects_of(w):
    return (np.arange(len(w.tmpls)) % 3).astype(np.int32)


@functools.lru_cache(maxsize=None)
def tset(name, kind, foot):
    from openfdcm_amd.engine import DeviceTemplates
    w = world(name)
    return DeviceTemplates(w.tmpls, line_caps=w.caps(kind), footprint=foot)


@functools.lru_cache(maxsize=None)
def shapes(name, n, margin, hull):
    w = world(name)
    return MO.Shapes(w.tmpls, w.recs[:n], w.base, margin, hull)


def run(name, kind, foot, n, permille=300, cross=None, margin=0, penalty=None, tau=1.0, objects=None, max_score=np.inf, min_matched=None,
        **kw):
    """(device, referee) of one call on the first n records."""
    w = world(name)
    objects = objects_of(w) if objects is None else objects
    got = w.dev.detect_matches_objects(tset(name, kind, foot), w.recs[:n], objects, max_score, overlap_permille=permille, cross_permille=cross,
                                       margin=margin, penalty=penalty, tau=tau, min_matched=min_matched, tmpl_index_base=w.base,
                                       indices=True, boxes=True, matched=True, **kw)
    ref_kw = {k: v for k, v in kw.items() if k in ("max_detections", "rescore")}
    want = MO.detect(w.tmpls, w.recs[:n], objects, tuple(a[:n] for a in w.ref(kind)), shapes(name, n, margin, foot == "hull"), w.base,
                     max_score=max_score, min_matched=min_matched, permille=permille, cross=cross,
                     den=None if penalty is None else R.denominators(w.tmpls, penalty, tau), **ref_kw)
    return got, want


def needs_shape(w, n):
    """The records of the first n that are valid, admissible and have lines."""
    t = w.recs["tmpl_idx"][:n].astype(np.int64) - w.base
    lines = np.array([x.shape[1] for x in w.tmpls])
    valid = (t >= 0) & (t < len(w.tmpls))
    return valid & w.ref()[4][:n] & (lines[np.clip(t, 0, len(w.tmpls) - 1)] > 0)


@pytest.mark.parametrize("margin", [0, 1, 3])
@pytest.mark.parametrize("name", MAPS)
def test_device_spans_equal_host_spans(name, margin):
    from openfdcm_amd.engine import lines_footprint_spans, match_footprint_spans
    w = world(name)
    n = 700
    mask = needs_shape(w, n)
    lines = np.array([x.shape[1] for x in w.tmpls])[np.clip(w.recs["tmpl_idx"].astype(np.int64) - w.base, 0, len(w.tmpls) - 1)]
    assert {1, 3, 64, 65, 130} <= set(lines[mask].tolist()) and mask.sum() > 300 and (~mask).sum() > 60
    off, spans, areas = w.dev.match_shapes(tset(name, "none", "box"), w.recs[:n], margin=margin, tmpl_index_base=w.base)
    # the host's table of every record, cut to the records the device builds
    hoff, hspans, hareas = match_footprint_spans(tset(name, "none", "box"), w.recs[:n], margin, tmpl_index_base=w.base)
    keep = np.concatenate([np.arange(hoff[j], hoff[j + 1]) for j in np.flatnonzero(mask)])
    rows = np.where(mask, np.diff(hoff), 0)
    assert off.dtype == np.int64 and np.array_equal(off, np.concatenate([[0], np.cumsum(rows)]))
    assert areas.dtype == np.int64 and np.array_equal(areas, np.where(mask, hareas, 0))
    assert spans.dtype == np.int32 and np.array_equal(spans, hspans[keep]), np.flatnonzero((spans != hspans[keep]).any(axis=1))[:5]
    assert (spans[:, 0] > spans[:, 1]).any() or margin > 0        # rows that pass between lattice points are empty
    if margin:
        assert 8 * 130 > 1024 and mask[lines == 130].any()        # more than 1024 vertices
    # the host's table against the referee's and against fdcm_lines_footprint_spans on the same posed lines
    m = min(n, 257)
    roff, rspans, rareas = shapes(name, m, margin, True).span_table()
    assert np.array_equal(hoff[:m + 1], roff) and np.array_equal(hspans[:roff[-1]], rspans) and np.array_equal(hareas[:m], rareas)
    posed = [R.posed(w.tmpls, r, w.base) for r in w.recs[:m]]
    loff, lspans, lareas = lines_footprint_spans([p if p is not None else np.zeros((4, 0), dtype=np.float32) for p in posed], margin=margin)
    assert np.array_equal(loff, roff) and np.array_equal(lspans, rspans) and np.array_equal(lareas, rareas)


def test_device_spans_of_degenerate_shapes():
    """One vertex (a zero-length line), a horizontal and a vertical line, a collinear triple, duplicate lines, a one-pixel
    square, under whole translations, quarter turns and free rotations."""
    from openfdcm_amd.engine import DeviceTemplates, match_footprint_spans
    w = world("adopted")
    tm = [np.float32([[2], [3], [2], [3]]), np.float32([[0], [4], [9], [4]]), np.float32([[4], [0], [4], [9]]),
          np.float32([[1, 5, 9], [1, 5, 9], [5, 9, 13], [5, 9, 13]]), np.float32([[1, 1, 8], [2, 2, 7], [8, 8, 1], [7, 7, 2]]),
          np.float32([[3, 4], [3, 3], [4, 3], [3, 4]])]
    rng = np.random.default_rng(12)
    M = []
    for i in range(96):
        a = [0.0, np.pi / 2, np.pi, rng.uniform(-np.pi, np.pi)][i % 4]
        c, s = np.cos(a), np.sin(a)
        M.append([c, -s, rng.integers(18, 40) + (0.5 if i % 8 == 7 else 0), s, c, rng.integers(14, 22)])
    M = np.float32(M)
    M[np.abs(M) < 1e-6] = 0
    recs = R.records(np.arange(96) % len(tm), np.zeros(96), M)
    ts = DeviceTemplates(tm)
    adm = R.verify(w.vol, w.keys, w.t, tm, recs)[4]
    assert adm.sum() > 40 and (adm & (np.arange(96) % len(tm) == 0)).any()
    for margin in (0, 2):
        off, spans, areas = w.dev.match_shapes(ts, recs, margin=margin)
        hoff, hspans, hareas = match_footprint_spans(ts, recs, margin)
        keep = np.concatenate([np.arange(hoff[j], hoff[j + 1]) for j in np.flatnonzero(adm)])
        assert np.array_equal(np.diff(off), np.where(adm, np.diff(hoff), 0)) and np.array_equal(areas, np.where(adm, hareas, 0))
        assert np.array_equal(spans, hspans[keep])
        roff, rspans, rareas = MO.Shapes(tm, recs, 0, margin, True, hull_ref.rows_by_pairs).span_table(adm)
        assert np.array_equal(off, roff) and np.array_equal(spans, rspans) and np.array_equal(areas, rareas)
    assert areas[adm & (np.arange(96) % len(tm) == 0)].min() == (2 * 2 + 1) ** 2     # one vertex and its margin


def test_a_tall_shape_is_read_from_memory_by_the_round():
    """A sliver of 1190 rows (more than the 1024 a workgroup stages) wins; a square inside its hull goes at overlap 0, a square
    inside its box and outside its hull stays: the unstaged path decides both."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates, match_footprint_spans
    rng = np.random.default_rng(4)
    keys = np.float32([-1.0, 0.5])
    vol = (rng.random((2, 16, 1200)) * 9).astype(np.float32)
    dev = DeviceFeatureMap.from_volume(keys, vol, (0.0, 0.0))
    tm = [np.float32([[1, 1], [1, 1], [14, 1], [1190, 1190]]), np.float32([[0, 2, 2, 0], [0, 0, 2, 2], [2, 2, 0, 0], [0, 2, 2, 0]])]
    recs = R.records([0, 1, 1], [1.0, 2.0, 3.0], [[1, 0, 0, 0, 1, 0], [1, 0, 2, 0, 1, 1000], [1, 0, 11, 0, 1, 100]])
    ver = R.verify(vol, keys, (0.0, 0.0), tm, recs)
    assert ver[4].all()
    for foot, kept in (("hull", [0, 2]), ("box", [0])):
        ts = DeviceTemplates(tm, footprint=foot)
        got = dev.detect_matches_objects(ts, recs, [0, 1], np.inf, overlap_permille=0, cross_permille=0, indices=True, boxes=True, matched=True)
        want = MO.detect(tm, recs, [0, 1], ver, MO.Shapes(tm, recs, 0, 0, foot == "hull"), permille=0, cross=0)
        assert same_detection(got, want) and list(got[1]) == kept
        assert got[2][0][3] - got[2][0][1] + 1 == 1190
    off, spans, areas = dev.match_shapes(ts, recs)
    hoff, hspans, hareas = match_footprint_spans(ts, recs)
    assert np.array_equal(off, hoff) and np.array_equal(spans, hspans) and np.array_equal(areas, hareas) and off[1] == 1190


@pytest.mark.parametrize("foot", ["box", "hull"])
@pytest.mark.parametrize("kind", MC.CAPS)
@pytest.mark.parametrize("name", MAPS)
def test_detect_equals_the_referee(name, kind, foot):
    kept = 0
    for permille, cross, margin in LIMITS:
        n = 257 if margin or permille == 1000 else 700       # (the referee's rule is quadratic in what it keeps)
        kws = [dict(), dict(max_score=MS, min_matched=MM, rescore=True, penalty=0)]
        if (permille, cross) == (300, 800):
            kws.append(dict(max_score=MS, min_matched=MM, penalty=1, tau=0.5))
        for kw in kws:
            got, want = run(name, kind, foot, n, permille=permille, cross=cross, margin=margin, max_detections=4096, **kw)
            assert same_detection(got, want), (permille, cross, margin, kw, len(got[0]), len(want[0]), got[1][:6], want[1][:6])
            kept += len(want[0])
    for n in (1, 255, 256):
        got, want = run(name, kind, foot, n, permille=300, cross=800)
        assert same_detection(got, want), n
    assert kept > 400


@pytest.mark.parametrize("max_detections", [1, 64, 65, 200])
def test_the_rounds_cross_a_batch(max_detections):
    got, want = run("lines", "none", "hull", 700, permille=1000, cross=1000, max_detections=max_detections)
    assert len(want[0]) == max_detections and same_detection(got, want)
    for foot in ("box", "hull"):
        got, want = run("lines", "scalar", foot, 700, permille=300, cross=800, penalty=0, max_detections=max_detections)
        assert same_detection(got, want)


def test_the_cases_discriminate():
    """Box against hull, and cross 300 against 800, give different lists: no parametrisation passes vacuously.  The counts are
    the referees' on the adopted world (tests/test_match_objects_definition.py)."""
    counts = {}
    for foot in ("box", "hull"):
        for permille, cross in ((300, 300), (300, 800), (0, 0)):
            got, want = run("adopted", "none", foot, 700, permille=permille, cross=cross)
            assert same_detection(got, want)
            counts[foot, permille, cross] = len(got[0])
    assert [counts["box", 300, 300], counts["hull", 300, 300]] == [70, 87]
    assert [counts["box", 300, 800], counts["hull", 300, 800]] == [89, 117]
    assert [counts["box", 0, 0], counts["hull", 0, 0]] == [27, 34]


def test_identity_1_one_object_on_a_box_set_is_matches_detect():
    w = world("lines")
    one = np.zeros(len(w.tmpls), dtype=np.int32)
    for kind in ("none", "mixed"):
        for kw in (dict(overlap_permille=300, penalty=0), dict(overlap_permille=0, margin=3), dict(overlap_permille=500, rescore=True, penalty=1, tau=0.5)):
            for ms, mm in ((np.inf, 0.0), (25.0, 0.5)):
                want = w.dev.detect_matches(tset("lines", kind, "box"), w.recs, max_score=ms, min_matched=mm, tmpl_index_base=w.base, indices=True,
                                            boxes=True, matched=True, **kw)
                for cross in (0, 1000):
                    got = w.dev.detect_matches_objects(tset("lines", kind, "box"), w.recs, one, ms, min_matched=mm, cross_permille=cross,
                                                       tmpl_index_base=w.base, indices=True, boxes=True, matched=True, **kw)
                    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)) and len(got[0]) > 3


def test_identity_2_cross_1000_is_the_merge_of_the_objects_own_lists():
    w = world("adopted")
    obj = objects_of(w)
    got = w.dev.detect_matches_objects(tset("adopted", "scalar", "box"), w.recs, obj, MS, min_matched=MM, overlap_permille=300, cross_permille=1000,
                                       max_detections=4096, tmpl_index_base=w.base, indices=True)
    merged = []
    t = w.recs["tmpl_idx"].astype(np.int64) - w.base
    valid = (t >= 0) & (t < len(w.tmpls))
    for o in range(3):
        own = np.array(w.recs)
        own["tmpl_idx"][valid & (obj[np.clip(t, 0, len(w.tmpls) - 1)] != o)] = w.base - 1
        d = w.dev.detect_matches(tset("adopted", "scalar", "box"), own, max_score=MS[o], min_matched=MM[o], overlap_permille=300,
                                 max_detections=4096, tmpl_index_base=w.base, indices=True)
        merged += [((int(q.view(np.uint32)) << 32) | int(j), int(j)) for q, j in zip(d[0]["score"], d[1])]
    assert [j for _, j in sorted(merged)] == list(got[1]) and len(got[1]) > 20


def test_identities_3_5_and_6_on_the_device():
    w = world("adopted")
    obj = objects_of(w)
    kw = dict(tmpl_index_base=w.base, indices=True, boxes=True, matched=True, max_detections=4096)
    for margin in (0, 3):        # 3: no suppression on a hull set gives the box set's records
        a, b = [w.dev.detect_matches_objects(tset("adopted", "none", f), w.recs, obj, np.inf, overlap_permille=1000, cross_permille=1000,
                                             margin=margin, **kw) for f in ("box", "hull")]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a[0]) > 300
    # 5: at overlap 0 no two returned shapes share a pixel; their boxes do
    got = w.dev.detect_matches_objects(tset("adopted", "none", "hull"), w.recs, obj, np.inf, overlap_permille=0, cross_permille=0, **kw)
    sh, seen = shapes("adopted", 700, 0, True), set()
    for j in got[1]:
        px = sh.shape(int(j)).pixels()
        assert px and not (px & seen)
        seen |= px
    assert any(R.overlaps(got[2][a], got[2][b], 0) for a in range(len(got[2])) for b in range(a))
    # 6: relabelling the objects by a bijection, the per-object arrays permuted alike
    perm = np.array([2, 0, 1], dtype=np.int32)
    ms2, mm2 = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    ms2[perm], mm2[perm] = MS, MM
    for f in ("box", "hull"):
        a = w.dev.detect_matches_objects(tset("adopted", "mixed", f), w.recs, obj, MS, min_matched=MM, cross_permille=800, **kw)
        b = w.dev.detect_matches_objects(tset("adopted", "mixed", f), w.recs, perm[obj], ms2, min_matched=mm2, cross_permille=800, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a[0]) > 10


def test_identity_4_shapes_that_hold_their_box_corners_are_boxes():
    from openfdcm_amd.engine import DeviceTemplates
    w = world("adopted")
    rng = np.random.default_rng(8)
    tmpls = []
    for n in (2, 5, 9):
        t = np.rint(rng.uniform(2, 20, size=(4, n))).astype(np.float32)
        x0, x1, y0, y1 = t[[0, 2]].min(), t[[0, 2]].max(), t[[1, 3]].min(), t[[1, 3]].max()
        tmpls.append(np.concatenate([t, np.array([[x0, x1], [y0, y1], [x1, x0], [y0, y1]], dtype=np.float32)], axis=1))
    forms = [[1, 0, 0, 0, 1, 0], [-1, 0, 0, 0, 1, 0], [1, 0, 0, 0, -1, 0], [-1, 0, 0, 0, -1, 0], [0, -1, 0, 1, 0, 0], [0, 1, 0, -1, 0, 0]]
    n = 60
    M = np.array([forms[i % 6] for i in range(n)], dtype=np.float32)
    M[:, 2], M[:, 5] = rng.integers(20, 40, size=n), rng.integers(12, 22, size=n)
    recs = R.records(rng.integers(0, 3, size=n), rng.uniform(0, 9, size=n), M)
    for margin in (0, 2):
        for permille, cross in ((300, 300), (100, 600), (0, 0)):
            a, b = [w.dev.detect_matches_objects(DeviceTemplates(tmpls, footprint=f), recs, [0, 1, 0], np.inf, overlap_permille=permille,
                                                 cross_permille=cross, margin=margin, indices=True, boxes=True, matched=True) for f in ("box", "hull")]
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and 0 < len(a[0]) < n


@pytest.mark.parametrize("foot", ["box", "hull"])
def test_identity_7_integer_translations_are_the_windows_call(foot):
    """The device-built shapes against the host-built shapes of the windows' path."""
    from openfdcm_amd.engine import DeviceTemplates
    w = world("adopted")
    tm = MC.template_set(9, integer=True)
    obj = (np.arange(len(tm)) % 3).astype(np.int32)
    rng = np.random.default_rng(3)
    n = 160
    tr = np.stack([rng.integers(-6, w.W - 14, size=n), rng.integers(-6, w.H - 14, size=n)], axis=1)
    ti = rng.integers(0, len(tm), size=n)
    recs = R.records(ti, np.zeros(n), [[1, 0, x, 0, 1, y] for x, y in tr])
    jobs = np.stack([ti, np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64), tr[:, 0], tr[:, 1], np.ones(n, dtype=np.int64),
                     np.ones(n, dtype=np.int64)], axis=1).astype(np.int32)
    total = 0
    for caps in (None, MC.caps_of(tm, "mixed")):
        ts = DeviceTemplates(tm, line_caps=caps, footprint=foot)
        for permille, cross, margin in ((300, 800, 0), (0, 0, 2), (150, 1000, 1)):
            kw = dict(overlap_permille=permille, cross_permille=cross, margin=margin, penalty=0, min_matched=[0.0, 0.2, 0.4], max_detections=4096)
            got = w.dev.detect_matches_objects(ts, recs, obj, [400.0, 300.0, np.inf], rescore=True, indices=True, boxes=True, matched=True, **kw)
            win = w.dev.exhaustive_detect_windows_objects(ts, jobs, obj, [400.0, 300.0, np.inf], boxes=True, matched=True, job_index=True, **kw)
            assert MC.same_records(got[0], win[0]) and np.array_equal(got[1], win[3]) and np.array_equal(got[2], win[1])
            assert MC.same_floats(got[3], win[2])
            total += len(got[0])
    assert total > 60


def test_identity_9_the_three_input_forms_and_two_runs():
    import torch
    import openfdcm_amd as fd
    from openfdcm_amd.engine import search_raw
    w = world("lines")
    obj = objects_of(w)
    raw = search_raw(w.dev, tset("lines", "none", "hull"), w.scene, 4, 4, 1, 10, 7)
    ver = R.verify(w.vol, w.keys, w.t, w.tmpls, raw, 7)
    den = R.denominators(w.tmpls, 0)
    want = MO.detect(w.tmpls, raw, obj, ver, MO.Shapes(w.tmpls, raw, 7, 0, True), 7, permille=300, cross=800, den=den)
    assert 0 < len(want[0]) < len(raw)
    kw = dict(overlap_permille=300, cross_permille=800, penalty=0, tmpl_index_base=7, indices=True, boxes=True, matched=True)
    buf = torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).copy()).cuda()
    for form in (dict(matches=None), dict(matches=raw), dict(matches=None, device_ptr=buf.data_ptr(), n=len(raw)), dict(matches=raw)):
        got = w.dev.detect_matches_objects(tset("lines", "none", "hull"), form.pop("matches"), obj, np.inf, **form, **kw)
        assert same_detection(got, want)
    off = w.dev.match_shapes(tset("lines", "none", "hull"), raw, tmpl_index_base=7)
    dof = w.dev.match_shapes(tset("lines", "none", "hull"), None, tmpl_index_base=7, device_ptr=buf.data_ptr(), n=len(raw))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(off, dof)) and off[0][-1] > 100
    # the public calls
    hull_list = fd.with_footprint(w.tmpls, "hull")
    pub = fd.detect_matches_objects(w.dev, hull_list, fd.MatchList(w.recs), obj, max_score=MS, overlap=0.3, cross_overlap=0.8,
                                    penalty=fd.DefaultPenalty(), min_matched=MM, return_indices=True, return_boxes=True, return_matched=True,
                                    return_objects=True)
    got, ref = run("lines", "none", "hull", 700, permille=300, cross=800, penalty=0, max_score=MS, min_matched=MM)
    assert same_detection((pub[0].records(), *pub[1:4]), ref) and np.array_equal(pub[4], obj[pub[0].records()["tmpl_idx"]])
    plain = fd.detect_matches_objects(w.dev, hull_list, w.recs, overlap=0.3)       # objects=None: hull shapes without labels
    one, ref1 = run("lines", "none", "hull", 700, permille=300, objects=np.zeros(len(w.tmpls), dtype=np.int32))
    assert isinstance(plain, fd.MatchList) and MC.same_records(plain.records(), ref1[0])
    tables = fd.match_footprint_spans(w.tmpls, w.recs[:40], margin=1), shapes("lines", 40, 1, True).span_table()
    assert all(np.array_equal(a, b) for a, b in zip(*tables))


def test_empty_inputs_and_the_refusals_that_need_handles():
    from openfdcm_amd import _capi
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates, match_footprint_spans
    w = world("adopted")
    obj = objects_of(w)
    none = np.zeros(0, dtype=R.MATCH_DTYPE)
    empty_map = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    for fm, ts, recs, ob in [(w.dev, tset("adopted", "none", "hull"), none, obj), (w.dev, DeviceTemplates([], footprint="hull"), w.recs[:5], []),
                             (empty_map, tset("adopted", "none", "hull"), w.recs[:5], obj)]:
        res = fm.detect_matches_objects(ts, recs, ob, np.inf, indices=True, boxes=True, matched=True)
        assert res[0].shape == (0,) and res[0].dtype == R.MATCH_DTYPE and res[1].shape == (0,) and res[2].shape == (0, 4) and res[3].shape == (0,)
        off, spans, areas = fm.match_shapes(ts, recs)
        assert not off.any() and len(off) == len(recs) + 1 and spans.shape == (0, 2) and not areas.any()
    assert match_footprint_spans(tset("adopted", "none", "box"), none)[0].tolist() == [0]
    for bad in ([0, 1, 2, 3, 0, 1, 2, 0, 1, 2], [0, 1, -1, 0, 1, 2, 0, 1, 2, 0]):
        with pytest.raises(_capi.FdcmError, match="objects: an entry is outside"):
            w.dev.detect_matches_objects(tset("adopted", "none", "box"), w.recs, bad, np.inf, n_objects=3, tmpl_index_base=w.base)
    # the one refusal behind GPU work: 9000 candidates of more than 8192 rows each at margin 4096
    adm = np.flatnonzero(needs_shape(w, 700))
    many = np.repeat(w.recs[adm[:1]], 9000)
    for call in (lambda: w.dev.detect_matches_objects(tset("adopted", "none", "hull"), many, obj, np.inf, margin=4096, tmpl_index_base=w.base),
                 lambda: w.dev.match_shapes(tset("adopted", "none", "hull"), many, margin=4096, tmpl_index_base=w.base)):
        with pytest.raises(_capi.FdcmError, match="cut the list with max_score or fdcm_topk first"):
            call()
    assert len(w.dev.detect_matches_objects(tset("adopted", "none", "box"), many, obj, np.inf, margin=4096, tmpl_index_base=w.base)) == 1
    got, want = run("adopted", "none", "hull", 257, permille=300, cross=800)     # the handle is as good as before
    assert same_detection(got, want)


def _probe(env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}
    out = subprocess.run([sys.executable, PROBE], capture_output=True, text=True, timeout=240, env={**clean, **env})
    assert out.returncode == 0, out.stdout + out.stderr
    return [l for l in out.stdout.splitlines() if l.startswith("match_objects_probe ")][-1].split()


def test_switches_and_poison_in_fresh_processes():
    """tools/match_objects_probe.py in fresh processes, one after another, each under its own time limit; nothing is started
    after a failure (an assertion ends the test).  The digests equal this process's own."""
    spec = __import__("importlib.util").util.spec_from_file_location("match_objects_probe", PROBE)
    probe = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    digest, rows, kept = probe.run()
    assert rows > 10000 and kept > 300
    for env in ({"FDCM_POISON": "0"}, {"FDCM_POISON": "1"}, {"FDCM_MATCHED_FLAT": "1"}, {"FDCM_FORCE_HOST_BINS": "1"}):
        line = _probe(env)
        assert line[1] == digest and int(line[3]) == rows and int(line[5]) == kept, (env, line)


def test_end_to_end_two_rods_and_a_washer_in_a_plate():
    """search -> detect_matches keeps one rod of two parallel rods at 45 degrees, detect_matches_objects on the hull list both;
    a washer inside a plate stays at cross_overlap 0.8 and goes at cross_overlap = overlap.  All equal the referees."""
    import openfdcm_amd as fd
    import match_objects_scene as S
    scene, tmpls, centres = S.two_rods()
    par = fd.Dt3CpuParameters(depth=S.DEPTH, dt3Coeff=S.COEFF, padding=S.PADDING)
    fm = fd.build_cpu_featuremap(scene, par)
    matches = fd.search(fd.DefaultMatch(), fd.DefaultSearch(S.MAX_TMPL, S.MAX_SCENE), fd.BatchOptimize(10), fm, tmpls, scene)
    dev, recs = fm._fm, matches.records()
    ver, den = R.verify(dev.volume(), dev.keys, dev.scene_translation, tmpls, recs, 0), R.denominators(tmpls, 0)
    kw = dict(max_score=S.ROD_MAX_SCORE, overlap=0.3, penalty=fd.DefaultPenalty(), return_indices=True, return_boxes=True, return_matched=True)
    box = fd.detect_matches(fm, tmpls, matches, **kw)
    want = R.detect(dev.volume(), dev.keys, dev.scene_translation, tmpls, recs, 0, max_score=S.ROD_MAX_SCORE, permille=300, den=den, verified=ver)
    assert same_detection((box[0].records(), *box[1:]), want) and len(box[0]) == 1
    hull = fd.detect_matches_objects(fm, fd.with_footprint(tmpls, "hull"), matches, **kw)
    want = MO.detect(tmpls, recs, [0], ver, MO.Shapes(tmpls, recs, 0, 0, True), max_score=S.ROD_MAX_SCORE, permille=300, den=den)
    assert same_detection((hull[0].records(), *hull[1:]), want) and len(hull[0]) == 2
    found = sorted(S.centre_of(tmpls[0], m.transform) for m in hull[0])
    assert all(np.hypot(f[0] - c[0], f[1] - c[1]) < 3.0 for f, c in zip(found, sorted(centres)))

    scene, tmpls, objects, centres = S.washer_in_plate()
    fm = fd.build_cpu_featuremap(scene, par)
    matches = fd.search(fd.DefaultMatch(), fd.DefaultSearch(S.MAX_TMPL, S.MAX_SCENE), fd.BatchOptimize(10), fm, tmpls, scene)
    dev, recs = fm._fm, matches.records()
    ver, den = R.verify(dev.volume(), dev.keys, dev.scene_translation, tmpls, recs, 0), R.denominators(tmpls, 0)
    for cross, kept in ((0.8, [0, 1]), (None, [0])):
        got = fd.detect_matches_objects(fm, tmpls, matches, objects, max_score=S.PLATE_MAX_SCORE, overlap=0.3, cross_overlap=cross,
                                        penalty=fd.DefaultPenalty(), return_indices=True, return_boxes=True, return_matched=True, return_objects=True)
        want = MO.detect(tmpls, recs, objects, ver, MO.Shapes(tmpls, recs, 0, 0, False), max_score=S.PLATE_MAX_SCORE, permille=300,
                         cross=300 if cross is None else 800, den=den)
        assert same_detection((got[0].records(), *got[1:4]), want) and list(got[4]) == kept
