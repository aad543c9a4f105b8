"""GPU tests of the detections suppressed by footprint overlap (include/fdcm.h, "Detections suppressed by footprint
overlap"): records and footprints against the numpy definition (nms_ref.py) applied to the device's own best-map planes,
the identity with fdcm_search_exhaustive_detect at radius 0, the large grid, degenerate grids, ties on an all-zero volume,
a known answer the radius rule cannot give, a capped set, determinism, and the public Python surface."""
import numpy as np
import pytest

from nms_ref import EMPTY, detect_nms_ref, footprints, nms_ref
from rotation_ref import rot_matrix
from test_gpu_detect import CS7, DEFAULT, EXPONENTIAL, ROTS, _centers, _cs, _same_records, built_pair, ragged  # noqa: F401
from test_gpu_exhaustive_peaks import GRIDS

pytestmark = pytest.mark.gpu

PERMILLES = (0, 100, 300, 500, 1000)


def _same(got, want, k=None):
    """(records, boxes) of the device against the referee's, cut to the first k."""
    rec, box = got
    wrec, wbox = want if k is None else (want[0][:k], want[1][:k])
    _same_records(rec, wrec)
    assert box.dtype == np.int32 and box.shape == wbox.shape and np.array_equal(box, wbox)


def _planes(dev, tset, grid, cs, pv, penalty, tau):
    scores, pairs = dev.best_map(tset, grid, cs, pv, penalty=penalty, tau=tau)
    scores.setflags(write=False)
    pairs.setflags(write=False)
    return scores, pairs


@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[1]])
@pytest.mark.parametrize("rot,penalty,tau", [("none", None, 1.0), ("seven", EXPONENTIAL, 1.5), ("one", DEFAULT, 1.0)])
def test_detections_against_the_definition(built_pair, ragged, grid, rot, penalty, tau):
    """Records and footprints equal nms_ref on the device's best-map planes, byte for byte, at every threshold, margin and
    k.  The referee runs once per (threshold, margin) with k = 64: the rule's first k detections do not depend on k."""
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    cs = ROTS[rot]
    pv = None if cs is None else piv
    A = 1 if cs is None else len(cs)
    scores, pairs = _planes(dev, tset, grid, cs, pv, penalty, tau)
    for margin in (0, 3):
        boxes = footprints(tmpls, cs, pv, margin).reshape(-1, 4)
        for permille in PERMILLES:
            want = detect_nms_ref(scores, pairs, boxes, grid, 64, permille, A, cs, pv)
            for k in (1, 8, 64):
                got = dev.exhaustive_detect_nms(tset, grid, cs, pv, k=k, overlap_permille=permille, margin=margin, penalty=penalty,
                                                tau=tau, boxes=True)
                _same(got, want, k)
            assert len(want[0]) >= 1 and np.all(np.diff(want[0]["score"]) >= 0)


def test_the_rule_is_not_the_radius(built_pair, ragged):
    """The inputs are no degenerate case for the rule: without rotations, ExponentialPenalty(1.5), GRIDS[0], margin 0 and
    k = 64 the list at every threshold below 1000 has at least 2 and fewer than 64 records of at least 3 templates, and it is
    not the list of the radius rule at rx = ry = 8."""
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    grid = GRIDS[0]
    scores, pairs = _planes(dev, tset, grid, None, None, EXPONENTIAL, 1.5)
    boxes = footprints(tmpls).reshape(-1, 4)
    radius = dev.exhaustive_detect(tset, grid, k=64, rx=8, ry=8, penalty=EXPONENTIAL, tau=1.5)
    for permille in (0, 100, 300, 500):
        rec, box = dev.exhaustive_detect_nms(tset, grid, k=64, overlap_permille=permille, penalty=EXPONENTIAL, tau=1.5, boxes=True)
        print("permille", permille, "records", len(rec), "templates", len(np.unique(rec["tmpl_idx"])), "radius records", len(radius))
        _same((rec, box), detect_nms_ref(scores, pairs, boxes, grid, 64, permille))
        assert 2 <= len(rec) < 64
        assert len(np.unique(rec["tmpl_idx"])) >= 3
        assert rec.tobytes() != radius.tobytes()
        assert len({(b[2] - b[0], b[3] - b[1]) for b in box.tolist()}) >= 3  # footprints of different sizes


@pytest.mark.parametrize("rot", ["none", "seven", "one"])
def test_threshold_1000_is_the_detect_call_at_radius_0(built_pair, ragged, rot):
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    cs = ROTS[rot]
    pv = None if cs is None else piv
    for grid in (GRIDS[0], GRIDS[1]):
        for k in (1, 8, 64):
            want = dev.exhaustive_detect(tset, grid, cs, pv, k=k, rx=0, ry=0, penalty=EXPONENTIAL, tau=1.5)
            assert len(want) == k
            for margin in (0, 7):
                got = dev.exhaustive_detect_nms(tset, grid, cs, pv, k=k, overlap_permille=1000, margin=margin, penalty=EXPONENTIAL,
                                                tau=1.5)
                assert got.tobytes() == want.tobytes()


def test_the_large_grid(built_pair, ragged):
    """467 x 459: 256 workgroups, full partial arrays, several runs of keys per workgroup."""
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    grid = GRIDS[2]
    scores, pairs = _planes(dev, tset, grid, None, None, EXPONENTIAL, 1.5)
    want = detect_nms_ref(scores, pairs, footprints(tmpls).reshape(-1, 4), grid, 64, 300)
    assert len(want[0]) > 8
    _same(dev.exhaustive_detect_nms(tset, grid, k=64, overlap_permille=300, penalty=EXPONENTIAL, tau=1.5, boxes=True), want)


def test_degenerate_grids(built_pair, ragged):
    """One point, one row, one column; a grid wholly outside every box (no records, nothing launched over an empty plane);
    a grid whose candidates run out before k."""
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    boxes = footprints(tmpls, CS7, piv).reshape(-1, 4)
    x0, y0, nx, ny, _, _ = GRIDS[0]
    cand = np.argwhere(dev.best_map(tset, GRIDS[0], CS7, piv, penalty=DEFAULT)[1] >= 0)
    j, i = cand[np.argmin(np.abs(cand - [ny // 2, nx // 2]).sum(axis=1))]  # a point with a candidate, near the middle
    cx, cy = x0 + int(i), y0 + int(j)
    for grid, some in [((cx, cy, 1, 1, 1, 1), True), ((cx, cy - 200, 1, 300, 1, 1), True), ((cx - 150, cy, 300, 1, 1, 1), True),
                       ((cx - 1, cy, 3, 2, 1, 1), True), ((cx - 150, cy - 3, 150, 1, 2, 3), True)]:
        scores, pairs = _planes(dev, tset, grid, CS7, piv, DEFAULT, 1.0)
        for permille in (0, 300, 1000):
            want = detect_nms_ref(scores, pairs, boxes, grid, 64, permille, len(CS7), CS7, piv)
            got = dev.exhaustive_detect_nms(tset, grid, CS7, piv, k=64, overlap_permille=permille, penalty=DEFAULT, boxes=True)
            print("grid", grid, "permille", permille, "records", len(got[0]), "candidates", int((pairs >= 0).sum()))
            _same(got, want)
            assert len(got[0]) <= (pairs >= 0).sum() and (not some or len(got[0]) > 0)
            if permille == 1000:  # the candidates run out before k = 64 on the small grids
                assert len(got[0]) == min(64, (pairs >= 0).sum())
    far = (5000, 5000, 40, 30, 1, 1)
    rec, box = dev.exhaustive_detect_nms(tset, far, CS7, piv, k=8, boxes=True)
    assert len(rec) == 0 and box.shape == (0, 4)
    assert len(dev.exhaustive_detect_nms(tset, far, k=8)) == 0


def test_all_zero_volume_ties():
    """Every q is 0, so the order is pure grid order: at threshold 0 the detections are the lattice the referee predicts,
    the first candidate point, then the first whose footprint is clear of it, and so on; both templates, whose boxes differ
    in size, occur."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    dev = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 40, 30), dtype=np.float32), (0.0, 0.0))
    tmpls = [np.array([[2, 3, 10, 12], [5, 5, 6, 20]], dtype=np.float32).T.copy(), np.array([[1, 1, 2, 2]], dtype=np.float32).T.copy()]
    tset = DeviceTemplates(tmpls)
    grid = (-5, -4, 37, 29, 1, 1)
    boxes = footprints(tmpls).reshape(-1, 4)
    assert boxes.tolist() == [[2, 3, 10, 20], [1, 1, 2, 2]]
    scores, pairs = _planes(dev, tset, grid, None, None, None, 1.0)
    assert np.all(scores[pairs >= 0] == 0) and set(np.unique(pairs)) == {-1, 0, 1}
    for permille in (0, 300, 1000):
        for k in (1, 7, 64):
            want = detect_nms_ref(scores, pairs, boxes, grid, k, permille)
            _same(dev.exhaustive_detect_nms(tset, grid, k=k, overlap_permille=permille, boxes=True), want)
    rec, box = dev.exhaustive_detect_nms(tset, grid, k=64, overlap_permille=0, boxes=True)
    g = ((rec["transform"][:, 5] - grid[1]) * grid[2] + (rec["transform"][:, 2] - grid[0])).astype(np.int64)
    assert 2 < len(rec) <= 64 and np.all(rec["score"] == 0) and np.all(np.diff(g) > 0)
    assert set(rec["tmpl_idx"].tolist()) == {0, 1}
    for a in range(len(box)):
        for c in range(a):  # no two footprints share a pixel
            assert min(box[a, 2], box[c, 2]) < max(box[a, 0], box[c, 0]) or min(box[a, 3], box[c, 3]) < max(box[a, 1], box[c, 1])
    # and the lattice is maximal: every candidate point left out (before the last detection: the list may be full) meets a
    # detection that comes before it in grid order
    F = boxes[np.where(pairs.reshape(-1) >= 0, pairs.reshape(-1), 0)].astype(np.int64)
    gi = np.arange(grid[2] * grid[3])
    F = F + np.stack([grid[0] + gi % grid[2], grid[1] + gi // grid[2]] * 2, axis=1)
    for p in np.flatnonzero(pairs.reshape(-1) >= 0):
        if p < g[-1] and p not in g:
            assert any(d < p and min(F[p, 2], F[d, 2]) >= max(F[p, 0], F[d, 0]) and min(F[p, 3], F[d, 3]) >= max(F[p, 1], F[d, 1])
                       for d in g)


def test_known_answer_two_plants_closer_than_the_radius():
    """One narrow template planted twice, the second copy 13 pixels to the right of the first: less than r = 16 grid steps,
    more than the template's width of 11 pixels, so the footprints are disjoint.  The overlap rule returns both plants as
    its two best detections, with score 0; the radius rule at rx = ry = 16 returns one of them."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    S, r = 256, 16
    shape = np.array([(0, 0, 0, 30), (0, 0, 10, 0), (10, 0, 10, 12), (0, 12, 10, 12)], dtype=np.float32)
    other = shape.copy()
    other[2:, 2:] += 7
    PA, PB = (100, 80), (113, 80)
    segs = [(0, 0, S / 8, 0), (S - 1, S - 1, S - 1 - S / 8, S - 1)]
    for P in (PA, PB):
        segs += [(x1 + P[0], y1 + P[1], x2 + P[0], y2 + P[1]) for x1, y1, x2, y2 in shape]
    dev = DeviceFeatureMap.build(np.array(segs, dtype=np.float32).T.copy(), depth=12, coeff=5.0, padding=1.0, distance=0)
    tmpls = [other.T.copy(), shape.T.copy(), np.zeros((4, 0), dtype=np.float32)]
    tset = DeviceTemplates(tmpls)
    grid = dev.exhaustive_window(tset, 1, 1).as_tuple()
    assert footprints(tmpls)[1, 0].tolist() == [0, 0, 10, 30]

    def near(rec, P):
        return (np.abs(rec["transform"][:, 2] - P[0]) <= 2) & (np.abs(rec["transform"][:, 5] - P[1]) <= 2)
    rec, box = dev.exhaustive_detect_nms(tset, grid, k=8, overlap_permille=300, boxes=True)
    scores, pairs = _planes(dev, tset, grid, None, None, None, 1.0)
    _same((rec, box), detect_nms_ref(scores, pairs, footprints(tmpls).reshape(-1, 4), grid, 8, 300))
    assert len(rec) > 2 and np.all(rec["score"][:2] == 0) and rec["tmpl_idx"][:2].tolist() == [1, 1]
    assert near(rec[:2], PA).sum() == 1 and near(rec[:2], PB).sum() == 1
    assert box[0, 2] < box[1, 0] or box[1, 2] < box[0, 0]
    radius = dev.exhaustive_detect(tset, grid, k=8, rx=r, ry=r)
    assert len(radius) > 0 and radius["score"][0] == 0
    assert (near(radius, PA) | near(radius, PB)).sum() == 1


def test_capped_set(built_pair, ragged):
    """Caps enter through the best map alone: a set with line_caps = 3.0 against the referee on its own capped planes."""
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    tmpls, _, piv = ragged
    capped = DeviceTemplates(tmpls, line_caps=3.0)
    grid = GRIDS[0]
    scores, pairs = _planes(dev, capped, grid, CS7, piv, DEFAULT, 1.0)
    plain = dev.best_map(ragged[1], grid, CS7, piv, penalty=DEFAULT)
    assert scores.tobytes() != plain[0].tobytes()
    want = detect_nms_ref(scores, pairs, footprints(tmpls, CS7, piv, 2).reshape(-1, 4), grid, 64, 300, len(CS7), CS7, piv)
    _same(dev.exhaustive_detect_nms(capped, grid, CS7, piv, k=64, overlap_permille=300, margin=2, penalty=DEFAULT, boxes=True), want)


def test_determinism_and_index_base(built_pair, ragged):
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    call = lambda base: dev.exhaustive_detect_nms(tset, GRIDS[1], CS7, piv, k=64, overlap_permille=300, margin=1, penalty=EXPONENTIAL,
                                                  tau=1.5, tmpl_index_base=base, boxes=True)
    first = call(0)
    assert len(first[0]) > 2
    for _ in range(2):
        again = call(0)
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    # the calls of the radius rule in between leave the result alone, and theirs is what it was
    radius = dev.exhaustive_detect(tset, GRIDS[1], CS7, piv, k=64, rx=3, ry=1, penalty=EXPONENTIAL, tau=1.5)
    assert call(0)[0].tobytes() == first[0].tobytes()
    assert dev.exhaustive_detect(tset, GRIDS[1], CS7, piv, k=64, rx=3, ry=1, penalty=EXPONENTIAL, tau=1.5).tobytes() == radius.tobytes()
    shifted = call(-7)
    assert np.array_equal(shifted[0]["tmpl_idx"], first[0]["tmpl_idx"] - 7) and np.array_equal(shifted[1], first[1])
    back = shifted[0].copy()
    back["tmpl_idx"] += 7
    assert back.tobytes() == first[0].tobytes()


def test_handle_footprints_equal_the_definition(ragged):
    """fdcm_templates_footprints on a handle: the referee's boxes and fdcm_lines_footprints', int for int."""
    from openfdcm_amd.engine import DeviceTemplates, lines_footprints
    tmpls, tset, piv = ragged
    scaled = CS7.copy()
    scaled[2] = [2, 0]
    for cs, pv in [(None, None), (CS7, piv), (scaled, piv), (CS7, None)]:
        for margin in (0, 5):
            got = tset.footprints(cs, pv, margin=margin)
            assert got.dtype == np.int32 and np.array_equal(got, footprints(tmpls, cs, pv, margin))
            assert np.array_equal(got, lines_footprints(tmpls, cs, pv, margin=margin))
    assert tset.footprints()[0, 0].tolist() == list(EMPTY)
    assert DeviceTemplates([]).footprints(CS7).shape == (0, 7, 4)


def test_public_api():
    """openfdcm.exhaustive_detect_nms on a feature map built from an image: a MatchList in ascending score; the boxes are
    template_footprints of the winning pairs plus the translation; overlap = 1 is exhaustive_detect(radius=0)."""
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceTemplates
    img = np.full((160, 200), 40, dtype=np.uint8)
    img[30:70, 25:85] = 200   # a 60 x 40 box
    img[90:140, 120:150] = 200  # a 30 x 50 box
    box = lambda w, h: np.array([(0, 0, w, 0), (w, 0, w, h), (w, h, 0, h), (0, h, 0, 0)], dtype=np.float32).T.copy()
    tmpls = [box(58, 38), np.zeros((4, 0), dtype=np.float32), box(28, 48), box(40, 40)]
    dt3 = fd.build_image_featuremap(img, fd.Dt3CpuParameters(depth=12, dt3Coeff=5.0, distance=fd.L2), threshold=60)
    dev, tset = dt3._fm, DeviceTemplates(tmpls)
    pen = fd.ExponentialPenalty(1.5)
    m, boxes = fd.exhaustive_detect_nms(dt3, tmpls, overlap=0.3, k=6, penalty=pen, margin=2, return_boxes=True)
    assert isinstance(m, fd.MatchList) and len(m) >= 2 and boxes.shape == (len(m), 4) and boxes.dtype == np.int32
    assert all(m[i].score <= m[i + 1].score for i in range(len(m) - 1))
    g = fd.exhaustive_window(dt3, tmpls)
    raw = dev.exhaustive_detect_nms(tset, g, k=6, overlap_permille=300, margin=2, penalty=EXPONENTIAL, tau=1.5, boxes=True)
    rec = m.records()
    assert rec.tobytes() == raw[0].tobytes() and np.array_equal(boxes, raw[1])
    fp = fd.template_footprints(tmpls, margin=2)
    t = np.stack([rec["transform"][:, 2], rec["transform"][:, 5]] * 2, axis=1).astype(np.int32)
    assert np.array_equal(boxes, fp[rec["tmpl_idx"], 0] + t)
    assert sorted(rec["tmpl_idx"][:2]) == [0, 2]  # the two boxes, each by its own template, near where it was drawn
    for r in rec[:2]:
        want = (25, 30) if r["tmpl_idx"] == 0 else (120, 90)
        assert abs(r["transform"][2] - want[0]) <= 3 and abs(r["transform"][5] - want[1]) <= 3
    assert isinstance(fd.exhaustive_detect_nms(dt3, tmpls), fd.MatchList)
    # with angles: the engine call on the rotation window, and the boxes of the winning (template, angle)
    angles = np.deg2rad([0, 90])
    cs, piv = _cs([0, 90]), _centers(tmpls)
    m, boxes = fd.exhaustive_detect_nms(dt3, tmpls, overlap=0.25, stride=2, k=5, penalty=pen, angles=angles, return_boxes=True)
    g = fd.rotation_window(dt3, tmpls, angles, stride=2)
    raw = dev.exhaustive_detect_nms(tset, g, cs, piv, k=5, overlap_permille=250, penalty=EXPONENTIAL, tau=1.5, boxes=True)
    rec = m.records()
    assert len(rec) >= 2 and rec.tobytes() == raw[0].tobytes() and np.array_equal(boxes, raw[1])
    fp = fd.template_footprints(tmpls, angles=angles)
    for r, b in zip(rec, boxes):
        a = 0 if r["transform"][0] == 1 else 1
        M = rot_matrix(cs[a, 0], cs[a, 1], *piv[r["tmpl_idx"]])
        tx, ty = int(round(float(r["transform"][2]) - float(M[0, 2]))), int(round(float(r["transform"][5]) - float(M[1, 2])))
        assert np.array_equal(b, fp[r["tmpl_idx"], a] + np.int32([tx, ty, tx, ty]))
    for kw in [dict(), dict(angles=angles, stride=2)]:
        one = fd.exhaustive_detect_nms(dt3, tmpls, overlap=1.0, k=7, penalty=pen, margin=9, **kw)
        assert one.records().tobytes() == fd.exhaustive_detect(dt3, tmpls, radius=0, k=7, penalty=pen, **kw).records().tobytes()
    win = (10, 12, 40, 30, 2, 2)
    m2 = fd.exhaustive_detect_nms(dt3, tmpls, overlap=0.5, k=2, window=win)
    assert m2.records().tobytes() == dev.exhaustive_detect_nms(tset, win, k=2, overlap_permille=500).tobytes()
    with pytest.raises(TypeError):
        fd.exhaustive_detect_nms(dt3, tmpls, penalty=1.5)
    with pytest.raises(fd._capi.FdcmError):
        fd.exhaustive_detect_nms(dt3, tmpls, overlap=1.2)
    wide = np.array([[-400.0, 0.0, dev.width + 400.0, 0.0]], dtype=np.float32).T.copy()
    m3, b3 = fd.exhaustive_detect_nms(dev, [wide], return_boxes=True)
    assert len(m3) == 0 and b3.shape == (0, 4)
    del dt3
    fd.clear_featuremap_pool()
