"""CPU-only: the end-to-end scenes of the match lists with objects and hull shapes (tests/match_objects_scene.py) give what
test_gpu_match_objects.py asks of the device.  On the oracle's match list the referees keep one rod of the two for the box
(tests/match_ref.py, overlap 0.3) and both for the hull (tests/match_objects_ref.py); and the washer inside the plate is kept
at cross_overlap 0.8 and dropped at cross_overlap = overlap."""
import numpy as np

import match_objects_ref as MO
import match_objects_scene as S
import match_ref as R
from oracle import oracle as O


def searched(scene, tmpls):
    orc = O.build(scene, depth=S.DEPTH, coeff=S.COEFF, padding=S.PADDING, distance=O.L2, nthreads=2)
    raw = O.search(orc, tmpls, scene, S.MAX_TMPL, S.MAX_SCENE, kind=O.BATCH_OPTIMIZE, batch=10, nthreads=2)
    return orc, raw, R.verify(orc.volume(), orc.keys, orc.translation, tmpls, raw, 0), R.denominators(tmpls, 0)


def test_two_rods_are_one_for_the_box_and_two_for_the_hull():
    scene, tmpls, centres = S.two_rods()
    orc, raw, ver, den = searched(scene, tmpls)
    q = raw["score"] / den[raw["tmpl_idx"]]
    cen = np.array([S.centre_of(tmpls[r["tmpl_idx"]], r["transform"]) for r in raw])
    per = [np.hypot(cen[:, 0] - c[0], cen[:, 1] - c[1]) for c in centres]
    assert len(raw) > 20 and max(q[d < 3].min() for d in per) < S.ROD_MAX_SCORE < q[np.min(per, axis=0) > 6].min()
    box = R.detect(orc.volume(), orc.keys, orc.translation, tmpls, raw, 0, max_score=S.ROD_MAX_SCORE, permille=300, den=den, verified=ver)
    assert len(box[0]) == 1
    same = MO.detect(tmpls, raw, [0], ver, MO.Shapes(tmpls, raw, 0, 0, False), max_score=S.ROD_MAX_SCORE, permille=300, den=den)
    assert np.array_equal(same[1], box[1])
    hull = MO.detect(tmpls, raw, [0], ver, MO.Shapes(tmpls, raw, 0, 0, True), max_score=S.ROD_MAX_SCORE, permille=300, den=den)
    assert len(hull[0]) == 2 and hull[1][0] == box[1][0]
    found = sorted(S.centre_of(tmpls[0], r["transform"]) for r in hull[0])
    assert all(np.hypot(f[0] - c[0], f[1] - c[1]) < 3.0 for f, c in zip(found, sorted(centres)))
    # the searched poses are pulled 2.8 pixels towards each other, so the two hulls touch: their overlap stays far below 0.3 of
    # their union, while their boxes overlap by more
    sh = MO.Shapes(tmpls, raw, 0, 0, True)
    a, b = sh.shape(int(hull[1][0])), sh.shape(int(hull[1][1]))
    inter = len(a.pixels() & b.pixels())
    assert 1000 * inter < 100 * (a.area + b.area - inter) and R.overlaps(hull[2][0], hull[2][1], 300)


def test_the_washer_in_the_plate_needs_the_cross_limit():
    scene, tmpls, objects, centres = S.washer_in_plate()
    orc, raw, ver, den = searched(scene, tmpls)
    kw = dict(max_score=S.PLATE_MAX_SCORE, permille=300, den=den)
    for hull in (False, True):
        both = MO.detect(tmpls, raw, objects, ver, MO.Shapes(tmpls, raw, 0, 0, hull), cross=800, **kw)
        assert sorted(both[0]["tmpl_idx"]) == [0, 1]
        for r, c in zip(sorted(both[0], key=lambda r: r["tmpl_idx"]), centres):
            f = S.centre_of(tmpls[r["tmpl_idx"]], r["transform"])
            assert np.hypot(f[0] - c[0], f[1] - c[1]) < 3.0
        one = MO.detect(tmpls, raw, objects, ver, MO.Shapes(tmpls, raw, 0, 0, hull), cross=300, **kw)
        assert len(one[0]) == 1 and one[1][0] == both[1][0]
