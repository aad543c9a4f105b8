"""CPU-only checks of the definition of the calls on match lists (include/fdcm.h, "Match lists"): the numpy referee
(match_ref.py) on a pyoracle.build map gives the answers worked out by hand for a one-line and a three-line template, obeys
the section's identities 2, 3 and 4, and its footprints are those of the posed lines in exact integers.  The rounding note
of the section is shown on one record: posing with the folded matrix and scoring at translation (0, 0) is not the search's
own arithmetic.  fdcm_matches_footprints takes a template handle, which a process without a device cannot make: the library's
footprints are compared with the referee's in test_gpu_matches.py, as fdcm_templates_footprints is in test_gpu_detect_nms.py."""
import functools
import math

import numpy as np
import pytest

import match_cases as MC
import match_ref as R
from nms_ref import box_of_lines
from oracle import pyoracle as P

f32 = np.float32


@functools.lru_cache(maxsize=None)
def the_map():
    """A 48 x 48 map of 6 slices with scene translation (0, 0)."""
    from openfdcm_amd import synthetic
    fm = P.build(synthetic.scene(48, 14, 3), depth=6, coeff=5.0, padding=1.0)
    assert fm["W"] == fm["H"] == 48 and len(fm["keys"]) == 6 and tuple(fm["t"]) == (0.0, 0.0)
    return fm


def verify(templates, recs, caps=None, base=0):
    fm = the_map()
    return R.verify(fm["vol"], fm["keys"], fm["t"], templates, recs, base, caps)


def test_a_one_line_template_by_hand():
    v = the_map()["vol"]
    tm = [np.float32([[0], [0], [10], [0]])]
    recs = R.records([0, 0, 0, 1, -1], [1, 1, 1, 1, 1], [[1, 0, 12.25, 0, 1, 20.5], [1, 0, -0.5, 0, 1, 47.75], [1, 0, 38.0, 0, 1, 3],
                                                        [1, 0, 12.25, 0, 1, 20.5], [1, 0, 12.25, 0, 1, 20.5]])
    s, f, c, ml, adm = verify(tm, recs)
    # record 0: (12.25, 20.5) - (22.25, 20.5), a horizontal line: key 0 of 6 keys from -pi/2 in steps of pi/6 is slice 3
    want = abs(f32(v[3, 12, 20] - v[3, 22, 20]))
    assert adm[0] and c[0, 0].tobytes() == want.tobytes() and s[0].tobytes() == want.tobytes() and f[0] == 1 and ml[0] == 10
    # record 1: x from -0.5 (inside (-1, W), pixel 0) to 9.5, y = 47.75 (pixel 47)
    want = abs(f32(v[3, 0, 47] - v[3, 9, 47]))
    assert adm[1] and c[1, 0].tobytes() == want.tobytes()
    # record 2: x reaches 48 = W: not admissible; records 3 and 4: tmpl_idx outside the set
    assert not adm[2] and np.isnan(s[2]) and np.isnan(f[2]) and np.isnan(c[2]).all()
    assert not adm[3] and not adm[4] and np.isnan(s[3:]).all() and np.isnan(c[3:]).all()
    assert np.array_equal(R.footprints(tm, recs, 0, 2), [[10, 18, 24, 22], [-3, 45, 11, 49], [36, 1, 50, 5], [0, 0, -1, -1], [0, 0, -1, -1]])
    # a cap below the cost: the score is the cap and nothing is matched; a cap of +inf matches whatever the cost
    cost = c[0, 0]
    assert cost > 0
    s2, f2, c2, ml2, _ = verify(tm, recs[:1], caps=[np.float32([cost / 2])])
    assert s2[0] == f32(cost / 2) and f2[0] == 0 and ml2[0] == 0 and c2[0, 0] == cost


def test_a_three_line_template_by_hand():
    v = the_map()["vol"]
    tm = [np.zeros((4, 0), dtype=np.float32), np.float32([[0, 0, 2], [0, 0, 1], [10, 0, 8], [0, 8, 3]])]
    # a quarter turn: (x, y) -> (30 - y, 5 + x)
    recs = R.records([8], [0], [[0, -1, 30, 1, 0, 5]])
    p = R.posed(tm, recs[0], 7)
    assert np.array_equal(p, np.float32([[30, 30, 29], [5, 5, 7], [30, 22, 27], [15, 5, 13]]))
    s, f, c, ml, adm = verify(tm, recs, base=7)
    # line 0 is vertical (dy / dx = +inf, atan = pi/2, which wraps to slice 0), line 1 horizontal (slice 3), line 2 has
    # dy / dx = 6 / -2, atan(-3) = -71.6 degrees, nearest to -60: slice 1
    want = [abs(f32(v[0, 30, 5] - v[0, 30, 15])), abs(f32(v[3, 30, 5] - v[3, 22, 5])), abs(f32(v[1, 29, 7] - v[1, 27, 13]))]
    assert adm[0] and np.array_equal(c[0], np.float32(want))
    assert s[0].tobytes() == f32(f32(want[0] + want[1]) + want[2]).tobytes()
    lens = np.float32([10, 8, math.sqrt(40)])
    assert f[0] == 1 and ml[0] == f32(f32(lens[0] + lens[1]) + lens[2])
    assert np.array_equal(R.footprints(tm, recs, 7, 0), [[22, 5, 30, 15]])
    # caps: line 1 alone capped at zero
    s2, f2, _, ml2, _ = verify(tm, recs, caps=[np.zeros(0, dtype=np.float32), np.float32([np.inf, 0, np.inf])], base=7)
    assert s2[0].tobytes() == f32(f32(want[0] + f32(0)) + want[2]).tobytes()
    matched = f32(f32(lens[0] + (lens[1] if want[1] == 0 else f32(0))) + lens[2])
    assert ml2[0] == matched and f2[0] == f32(matched / f32(f32(lens[0] + lens[1]) + lens[2]))
    # the template without lines: admissible, +0, fraction 1, the empty box, and never a candidate
    e = R.records([7], [0], [[1, 0, 1e9, 0, 1, 1e9]])
    s3, f3, _, _, adm3 = verify(tm, e, base=7)
    assert adm3[0] and s3[0].tobytes() == f32(0).tobytes() and f3[0] == 1 and tuple(R.footprints(tm, e, 7, 3)[0]) == (0, 0, -1, -1)
    fm = the_map()
    assert len(R.detect(fm["vol"], fm["keys"], fm["t"], tm, e, 7)[0]) == 0


@functools.lru_cache(maxsize=None)
def the_list():
    fm = the_map()
    tm = MC.template_set()[:7]
    recs = MC.record_list(5, fm["W"], fm["H"], fm["t"], tm, 300)
    return tm, recs, R.verify(fm["vol"], fm["keys"], fm["t"], tm, recs)


def detect(**kw):
    fm = the_map()
    tm, recs, ver = the_list()
    return R.detect(fm["vol"], fm["keys"], fm["t"], tm, recs, 0, verified=ver, **kw)


def test_identity_2_a_threshold_returns_the_leading_records():
    full = detect(permille=300)
    assert len(full[0]) > 5
    for ms in (0.0, 3.0, 11.5, 20.0, np.inf):
        part = detect(permille=300, max_score=ms)
        k = int((full[0]["score"] <= f32(ms)).sum())
        assert len(part[0]) == k and all(np.array_equal(a, b[:k]) for a, b in zip(part[1:3], full[1:3]))
        assert MC.same_records(part[0], full[0][:k])
    assert np.all(np.diff(full[0]["score"]) >= 0)


def test_identity_3_at_overlap_0_no_two_boxes_share_a_pixel():
    for margin in (0, 4):
        _, idx, B, _ = detect(permille=0, margin=margin)
        assert len(idx) > 1
        for a in range(len(B)):
            for b in range(a):
                assert not (max(B[a, 0], B[b, 0]) <= min(B[a, 2], B[b, 2]) and max(B[a, 1], B[b, 1]) <= min(B[a, 3], B[b, 3]))


def test_identity_4_a_duplicate_is_returned_only_at_overlap_1000():
    tm, recs, _ = the_list()
    for permille in (0, 300, 999, 1000):
        _, idx, _, _ = detect(permille=permille, max_detections=4096)
        kept = [recs[j].tobytes() for j in idx]
        assert (len(set(kept)) < len(kept)) == (permille == 1000), permille
    # the rule in Python integers, box by box, gives the same list
    fm = the_map()
    s, fr, _, ml, adm = the_list()[2]
    F = R.footprints(tm, recs, 0, 0)
    left = {j: (int(recs["score"][j:j + 1].view(np.uint32)[0]) << 32) | j for j in range(len(recs))
            if adm[j] and 0 <= recs["tmpl_idx"][j] < len(tm) and tm[recs["tmpl_idx"][j]].shape[1] and recs["score"][j] >= 0
            and not np.signbit(recs["score"][j])}
    out = []
    while left:
        d = min(left, key=left.get)
        del left[d]
        out.append(d)
        for g in [g for g in left if R.overlaps(F[g], F[d], 250)]:
            del left[g]
    assert np.array_equal(detect(permille=250, max_detections=4096)[1], out)


def test_footprints_are_the_posed_lines_in_exact_integers():
    tm, recs, _ = the_list()
    for margin in (0, 3):
        F = R.footprints(tm, recs, 0, margin)
        for j, r in enumerate(recs):
            p = R.posed(tm, r, 0)
            if p is None or p.shape[1] == 0 or np.isnan(p).any():
                assert tuple(F[j]) == (0, 0, -1, -1)
                continue
            assert np.array_equal(F[j], box_of_lines(p, margin))
            xs, ys = [float(x) for x in np.concatenate([p[0], p[2]])], [float(y) for y in np.concatenate([p[1], p[3]])]
            lim = 1 << 25
            clamp = lambda v: min(max(v, -lim), lim)   # noqa: E731
            if all(math.isfinite(x) for x in xs + ys):
                assert tuple(F[j]) == (clamp(math.floor(min(xs)) - margin), clamp(math.floor(min(ys)) - margin),
                                       clamp(math.floor(max(xs)) + margin), clamp(math.floor(max(ys)) + margin))
    inf = R.records([3, 3], [0, 0], [[1, 0, np.inf, 0, 1, 2], [1, 0, 5, 0, 1, -np.inf]])
    F = R.footprints(tm, inf, 0, 1)
    assert F[0, 0] == F[0, 2] == 1 << 25 and F[1, 1] == F[1, 3] == -(1 << 25)        # an infinity clamps, it does not empty the box


def test_the_rounding_note_s_is_not_the_search_score():
    """The search scores transform(lines, A) at a translation k v and stores A with the translation folded in; s(r) poses with
    the folded matrix.  One record where the two differ; both are finite, and nothing else is claimed."""
    fm = the_map()
    # x1 = 0.31183144, A's translation 18.46653 and the search's translation 6.2216387 along x: (x1 + 18.46653) + 6.2216387 is
    # 25.0 in float32 and x1 + (18.46653 + 6.2216387) is 24.999998: the end point is read at pixel 25 by the search, at 24 here
    tm = [np.float32([[0.31183144450187683], [0.2], [9.7], [0.4]])]
    A = np.float32([[1, 0, 18.466529846191406], [0, 1, 14]])
    k = f32(6.2216386795043945)
    lines = P.transform(tm[0], A)                                  # the search's posed lines
    bins = [P.closest_orientation(fm["keys"], lines[:, 0])]
    M = A.copy()
    M[0, 2] = f32(A[0, 2] + k)                                     # the record's matrix: the translation folded in
    assert int(f32(lines[0, 0] + k)) == 25 and int(R.posed(tm, R.records([0], [0], [M.reshape(6)])[0])[0, 0]) == 24
    search_score = P.evaluate(fm, lines, bins, (k, f32(0)))
    s = verify(tm, R.records([0], [search_score], [M.reshape(6)]))[0][0]
    assert np.isfinite(s) and np.isfinite(search_score)
