"""End to end: search -> the detect rule at overlap 1 -> scene selection on the notch scene (tests/match_coverage_scene.py), the
L-shaped part with the bar in its notch.  On the CPU with the oracle's match list and the referees; on the GPU the same chain
through the public calls, on a map built from the frame (with the bar a pixel further out: match_coverage_scene.py says why), equal
to the referee on the device's own records."""
import numpy as np
import pytest

import edge_ref
import match_coverage_ref as MC
import match_coverage_scene as S
import match_ref as R
import select_cases as SC
from oracle import oracle as O


def test_the_selection_keeps_the_part_and_the_bar_and_the_box_rule_loses_one():
    tm, scene = S.templates(), S.scene_lines()
    orc = O.build(scene, depth=30, coeff=5.0, padding=2.2, distance=O.L2, nthreads=2)
    raw = O.search(orc, tm, scene, S.MAX_TMPL, S.MAX_SCENE, kind=O.BATCH_OPTIMIZE, batch=10, nthreads=2)
    den = R.denominators(tm, 0)
    order = R.detect(orc.volume(), orc.keys, orc.translation, tm, raw, 0, permille=1000, den=den, max_detections=4096)[0]
    assert len(raw) == 60 and len(order) == 60 and np.all(np.diff(order["score"]) >= 0)
    labels = edge_ref.edge_labels(S.frame(), 30, 60)
    assert np.array_equal(S.frame(), SC.notch_frame())
    keys = edge_ref.keys_of(30)
    on = S.parts_of(order)
    for share in S.SHARES:
        sel, counts, res = MC.select(labels, keys, (0, 0), 160, 120, tm, order, 0, radius=2, bin_tolerance=1, min_new=share)
        assert sorted(on[j] for j in sel) == [0, 1], (share, sel, counts)                       # exactly two records, one on each part
        assert sel.tolist() == [0, 4] and counts.tolist() == [[42, 38, 38], [184, 137, 136]]
    box = R.detect(orc.volume(), orc.keys, orc.translation, tm, raw, 0, permille=S.BOX_OVERLAP, den=den)[0]
    kept = [k for k in S.parts_of(box) if k >= 0]
    assert len(set(kept)) == 1 and len(box) > 2, S.parts_of(box)                                 # the box rule loses a part and keeps junk


@pytest.mark.gpu
def test_the_same_chain_on_the_device():
    import openfdcm_amd as fd
    tm, scene, img = S.templates(), S.scene_lines(S.BAR_AT_IMAGE), S.frame(S.BAR_AT_IMAGE)
    labels = fd.edge_labels(img, depth=30, threshold=60)
    assert np.array_equal(labels, edge_ref.edge_labels(img, 30, 60))
    fm = fd.build_image_featuremap(img, threshold=60)
    matches = fd.search(fd.DefaultMatch(), fd.DefaultSearch(S.MAX_TMPL, S.MAX_SCENE), fd.BatchOptimize(10), fm, tm, scene)
    order = fd.detect_matches(fm, tm, matches, overlap=1.0, penalty=fd.DefaultPenalty(), max_detections=4096)
    assert len(order) > 20
    recs, dev = order.records(), fm._fm
    on = S.parts_of(recs, S.BAR_AT_IMAGE)
    for share in S.SHARES:
        got = fd.select_matches(fm, labels, tm, order, radius=2, bin_tolerance=1, min_new=share, return_residual=True)
        want = MC.select(labels, dev.keys, (0, 0), dev.width, dev.height, tm, recs, 0, radius=2, bin_tolerance=1, min_new=share)
        assert all(np.asarray(g).dtype == v.dtype and np.asarray(g).tobytes() == v.tobytes() for g, v in zip(got, want))
        assert sorted(on[j] for j in got[0]) == [0, 1], (share, got[0], got[1])
        parts = order[got[0]]
        assert isinstance(parts, fd.MatchList) and len(parts) == 2
