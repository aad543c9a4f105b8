"""The referee of the match lists with objects and hull shapes (tests/match_objects_ref.py) against the section's own
identities (include/fdcm.h, "Match lists: objects and hull shapes"), on match_cases' adopted world: no device.  Identities 1 to
6 and 8; 7 and 9 need the device (tests/test_gpu_match_objects.py).  Then the shapes: the referee's rows from the hull's edges
against hull_ref's two statements, and its span table of posed lines against fdcm_lines_footprint_spans on the same posed
lines.  fdcm_matches_footprint_spans takes a template handle, which a process without a device cannot make: it is held against
both in tests/test_gpu_match_objects.py, as fdcm_matches_footprints is in test_gpu_matches.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import hull_ref
import match_cases as MC
import match_objects_ref as MO
import match_ref as R

BASE = 5
N = 257


@functools.lru_cache(maxsize=None)
def world():
    keys, vol, t = MC.adopted_volume()
    tmpls = MC.template_set()
    recs = MC.record_list(77, vol.shape[1], vol.shape[2], t, tmpls, 700, BASE)
    ver = R.verify(vol, keys, t, tmpls, recs, BASE)
    return dict(keys=keys, vol=vol, t=t, tmpls=tmpls, recs=recs, ver=ver, objects=np.arange(len(tmpls)) % 3)


@functools.lru_cache(maxsize=None)
def shapes(n, margin, hull):
    w = world()
    return MO.Shapes(w["tmpls"], w["recs"][:n], BASE, margin, hull)


def run(n=N, margin=0, hull=True, objects=None, **kw):
    w = world()
    objects = w["objects"] if objects is None else objects
    return MO.detect(w["tmpls"], w["recs"][:n], objects, tuple(a[:n] for a in w["ver"]), shapes(n, margin, hull), BASE, **kw)


def same(a, b):
    return MC.same_records(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and MC.same_floats(a[3], b[3])


def test_the_cases_discriminate_as_the_issue_counted_them():
    """700 records, q = r.score, objects t % 3: box against hull 70 / 87 at (300, 300, 0), 89 / 117 at (300, 800, 0), 27 / 34 at
    (0, 0, 0)."""
    for (permille, cross), (nb, nh) in {(300, 300): (70, 87), (300, 800): (89, 117), (0, 0): (27, 34)}.items():
        b = run(700, hull=False, permille=permille, cross=cross)
        h = run(700, hull=True, permille=permille, cross=cross)
        assert (len(b[0]), len(h[0])) == (nb, nh), (permille, cross, len(b[0]), len(h[0]))


def test_identity_1_one_object_on_a_box_set_is_matches_detect():
    w = world()
    one = np.zeros(len(w["tmpls"]), dtype=np.int64)
    for kw in (dict(permille=300), dict(permille=0, max_score=25.0), dict(permille=500, min_matched=0.5, rescore=True, max_score=40.0)):
        for margin in (0, 3):
            want = R.detect(w["vol"], w["keys"], w["t"], w["tmpls"], w["recs"][:N], BASE, margin=margin,
                            verified=tuple(a[:N] for a in w["ver"]), **{"min_matched": 0.0, **kw})
            for cross in (0, 1000):
                assert same(run(margin=margin, hull=False, objects=one, cross=cross, **kw), want), (kw, margin, cross)
    assert len(want[0]) > 5


def test_identity_2_cross_1000_is_the_merge_of_the_objects_own_lists():
    w = world()
    recs = w["recs"][:N]
    got = run(hull=False, permille=300, cross=1000, max_score=[30.0, 20.0, 35.0], min_matched=[0.0, 0.3, 0.0])
    merged = []
    for o, (ms, mm) in enumerate(zip([30.0, 20.0, 35.0], [0.0, 0.3, 0.0])):
        own = np.array(recs)
        t = own["tmpl_idx"].astype(np.int64) - BASE
        other = (t >= 0) & (t < len(w["tmpls"])) & (w["objects"][np.clip(t, 0, len(w["tmpls"]) - 1)] != o)
        own["tmpl_idx"][other] = BASE - 1
        ver = R.verify(w["vol"], w["keys"], w["t"], w["tmpls"], own, BASE)
        d = R.detect(w["vol"], w["keys"], w["t"], w["tmpls"], own, BASE, max_score=ms, min_matched=mm, permille=300, verified=ver)
        merged += [((int(q.view(np.uint32)) << 32) | int(j), int(j)) for q, j in zip(d[0]["score"], d[1])]
    assert [j for _, j in sorted(merged)] == list(got[1]) and len(got[1]) > 20


def test_identity_3_no_suppression_on_a_hull_set_is_the_box_set():
    for margin in (0, 3):
        assert same(run(margin=margin, hull=True, permille=1000, cross=1000), run(margin=margin, hull=False, permille=1000, cross=1000))


def test_identity_4_shapes_that_hold_their_box_corners_are_boxes():
    """Templates that hold the corners of their box as end points, under {+-1, 0, x, 0, +-1, y} and exact quarter turns."""
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
    keys, vol, t = MC.adopted_volume()
    ver = R.verify(vol, keys, t, tmpls, recs)
    assert ver[4].sum() > 30
    for margin in (0, 2):
        for permille, cross in ((300, 300), (100, 600), (0, 0)):
            res = [MO.detect(tmpls, recs, [0, 1, 0], ver, MO.Shapes(tmpls, recs, 0, margin, hull), permille=permille, cross=cross)
                   for hull in (False, True)]
            assert same(*res) and 0 < len(res[0][0]) < ver[4].sum()


def test_identity_5_no_two_hull_shapes_share_a_pixel_at_overlap_0():
    got = run(700, hull=True, permille=0, cross=0)
    sh = shapes(700, 0, True)
    seen = set()
    for j in got[1]:
        px = sh.shape(int(j)).pixels()
        assert px and not (px & seen)
        seen |= px
    boxes = got[2].astype(np.int64)
    assert any(R.overlaps(boxes[a], boxes[b], 0) for a in range(len(boxes)) for b in range(a))  # their boxes do


def test_identity_6_relabelling_the_objects_changes_nothing():
    w = world()
    perm = np.array([2, 0, 1])
    ms, mm = np.array([30.0, 20.0, 35.0], dtype=np.float32), np.array([0.0, 0.3, 0.6], dtype=np.float32)
    a = run(permille=300, cross=800, max_score=ms, min_matched=mm)
    ms2, mm2 = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    ms2[perm], mm2[perm] = ms, mm
    b = run(permille=300, cross=800, objects=perm[w["objects"]], max_score=ms2, min_matched=mm2)
    assert same(a, b) and len(a[0]) > 10


def test_identity_8_a_threshold_cuts_the_list_of_no_threshold():
    full = run(permille=300, cross=800)
    for ms in (0.0, 7.5, 21.0):
        cut = run(permille=300, cross=800, max_score=ms)
        k = int((full[0]["score"] <= np.float32(ms)).sum())
        assert same(cut, tuple(a[:k] for a in full)) and np.all(full[0]["score"][:k] <= np.float32(ms))


def test_rows_from_the_hull_edges_are_the_rows_of_both_statements():
    w = world()
    seen = set()
    for j, r in enumerate(w["recs"][:120]):
        p = R.posed(w["tmpls"], r, BASE)
        if p is None or p.shape[1] > 9 or np.isnan(p).any() or np.isinf(p).any():
            continue
        for margin in (0, 2):
            v = hull_ref.vertices(p, margin)
            a, b, c = MO.rows_by_edges(v), hull_ref.rows_by_pairs(v), hull_ref.rows_by_halfplanes(v)
            assert hull_ref._same_rows(a, b) and hull_ref._same_rows(a, c), (j, margin)
        seen.add(p.shape[1])
    assert seen >= {1, 3, 4, 8, 9}
    # one vertex, a horizontal, a vertical and a zero-length line, collinear triples and duplicates
    for lines in ([[2.5], [3.5], [2.9], [3.1]], [[0], [4], [9], [4]], [[4], [0], [4], [9]], [[1, 5, 9, 1], [1, 5, 9, 1], [5, 9, 13, 5], [5, 9, 13, 5]]):
        v = hull_ref.vertices(np.array(lines, dtype=np.float32))
        assert hull_ref._same_rows(MO.rows_by_edges(v), hull_ref.rows_by_pairs_exact(v))


@pytest.mark.parametrize("margin", [0, 1, 3])
def test_the_span_table_of_posed_lines_is_the_librarys(margin):
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    from openfdcm_amd.engine import lines_footprint_spans
    w = world()
    n = 64 if margin else 257
    posed = [R.posed(w["tmpls"], r, BASE) for r in w["recs"][:n]]
    posed = [p if p is not None else np.zeros((4, 0), dtype=np.float32) for p in posed]
    off, spans, areas = shapes(n, margin, True).span_table()
    goff, gspans, gareas = lines_footprint_spans(posed, margin=margin)
    assert np.array_equal(off, goff) and np.array_equal(spans, gspans) and np.array_equal(areas, gareas) and off[-1] > 500
