"""GPU tests of "all detections below a score" (include/fdcm.h): records and footprints against the numpy definition
(detect_all_ref.py) applied to the device's own best-map planes, at thresholds taken from the data; the identity with
fdcm_search_exhaustive_detect_nms at +inf; lists of more than 64 records and lists that end at a batch boundary of the
rounds; thresholds at which most waves leave a template early and +inf at which none does; infinite and NaN values in the
volume; a capped set; ties on an all-zero volume; degenerate inputs; determinism and the public Python surface."""
import numpy as np
import pytest

from detect_all_ref import detect_all_ref
from nms_ref import footprints
from peaks_ref import NO_KEY, keys
from test_gpu_detect import CS7, DEFAULT, EXPONENTIAL, _same_records, built_pair, ragged  # noqa: F401
from test_gpu_exhaustive_peaks import GRIDS

pytestmark = pytest.mark.gpu

f32 = np.float32
INF = float("inf")


def _same(got, want):
    rec, box = got
    _same_records(rec, want[0])
    assert box.dtype == np.int32 and box.shape == want[1].shape and np.array_equal(box, want[1])


def _planes(dev, tset, grid, cs, pv, penalty, tau):
    scores, pairs = dev.best_map(tset, grid, cs, pv, penalty=penalty, tau=tau)
    scores.setflags(write=False)
    pairs.setflags(write=False)
    return scores, pairs


def _thresholds(L):
    """L[j].score for j in {0, len // 2, last}, the float below each, and 0 (a threshold below +0 is no argument)."""
    out = [f32(0)]
    for j in (0, len(L) // 2, len(L) - 1):
        s = f32(L["score"][j])
        out += [s, np.nextafter(s, f32(-np.inf))]
    return [t for t in out if t >= 0]


@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[1]])
@pytest.mark.parametrize("rot", ["none", "seven"])
@pytest.mark.parametrize("penalty,tau", [(DEFAULT, 1.0), (EXPONENTIAL, 1.5)])
def test_detections_against_the_definition(built_pair, ragged, grid, rot, penalty, tau):
    """Records and boxes equal detect_all_ref on the device's best-map planes, byte for byte, at every overlap, margin and
    threshold; at every threshold the count is what the prefix identity predicts from the list at +inf."""
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    cs, pv = (None, None) if rot == "none" else (CS7, piv)
    A = 1 if cs is None else len(cs)
    scores, pairs = _planes(dev, tset, grid, cs, pv, penalty, tau)
    md = 96
    for margin in (0, 3):
        boxes = footprints(tmpls, cs, pv, margin).reshape(-1, 4)
        for permille in (0, 300, 1000):
            call = lambda ms: dev.exhaustive_detect_all(tset, grid, cs, pv, max_score=ms, max_detections=md, overlap_permille=permille,
                                                        margin=margin, penalty=penalty, tau=tau, boxes=True)
            L = call(INF)
            _same(L, detect_all_ref(scores, pairs, boxes, grid, INF, md, permille, A, cs, pv))
            assert len(L[0]) >= 2 and np.all(np.diff(L[0]["score"]) >= 0)
            for ms in _thresholds(L[0]):
                got = call(ms)
                count = int((L[0]["score"] <= ms).sum())
                print("permille", permille, "margin", margin, "max_score", ms, "records", len(got[0]), "of", len(L[0]))
                assert len(got[0]) == count
                assert got[0].tobytes() == L[0][:count].tobytes() and np.array_equal(got[1], L[1][:count])
                _same(got, detect_all_ref(scores, pairs, boxes, grid, ms, md, permille, A, cs, pv))


@pytest.mark.parametrize("rot", ["none", "seven"])
def test_inf_is_the_nms_call(built_pair, ragged, rot):
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    cs, pv = (None, None) if rot == "none" else (CS7, piv)
    for grid in (GRIDS[0], GRIDS[1]):
        for k in (1, 8, 64):
            for permille, margin in [(300, 0), (0, 2), (1000, 0)]:
                want = dev.exhaustive_detect_nms(tset, grid, cs, pv, k=k, overlap_permille=permille, margin=margin, penalty=EXPONENTIAL,
                                                 tau=1.5, boxes=True)
                got = dev.exhaustive_detect_all(tset, grid, cs, pv, max_score=INF, max_detections=k, overlap_permille=permille,
                                                margin=margin, penalty=EXPONENTIAL, tau=1.5, boxes=True)
                assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])


def _smallest_keys(scores, pairs, grid, n, max_score=INF):
    """The records of the n smallest keys of the plane among the points with score <= max_score: overlap 1000 suppresses
    nothing."""
    from detect_ref import records
    kk = keys(scores).reshape(-1)
    with np.errstate(invalid="ignore"):
        kk = np.where(scores.reshape(-1) <= f32(max_score), kk, NO_KEY)
    order = np.sort(kk[kk != NO_KEY])[:n]
    g = (order & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return records(g, scores.reshape(-1)[g], pairs, 1, None, None, grid)


def test_more_than_64_detections(built_pair, ragged):
    """Overlap 1000 on GRIDS[0]: max_detections of 65, 128 and 200 give the smallest keys of the plane in order; with
    max_score the score of record 63, 64 and 127 the list ends at or next to a boundary of the batches of 64 rounds."""
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    grid = GRIDS[0]
    scores, pairs = _planes(dev, tset, grid, None, None, EXPONENTIAL, 1.5)
    full = _smallest_keys(scores, pairs, grid, 200)
    assert len(full) == 200
    for md in (65, 128, 200):
        got = dev.exhaustive_detect_all(tset, grid, max_score=INF, max_detections=md, overlap_permille=1000, penalty=EXPONENTIAL, tau=1.5)
        _same_records(got, full[:md])
        for j in (63, 64, 127):
            ms = full["score"][j]
            want = _smallest_keys(scores, pairs, grid, md, ms)
            got = dev.exhaustive_detect_all(tset, grid, max_score=ms, max_detections=md, overlap_permille=1000, penalty=EXPONENTIAL,
                                            tau=1.5)
            print("max_detections", md, "threshold of record", j, "records", len(got))
            assert len(want) >= min(md, j + 1)
            _same_records(got, want)


def test_the_large_grid_to_the_end_of_the_list(built_pair, ragged):
    """GRIDS[2] (467 x 459), overlap 300, max_detections 4096: the list runs until the points run out."""
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    grid = GRIDS[2]
    scores, pairs = _planes(dev, tset, grid, None, None, EXPONENTIAL, 1.5)
    boxes = footprints(tmpls).reshape(-1, 4)
    got = dev.exhaustive_detect_all(tset, grid, max_score=INF, max_detections=4096, overlap_permille=300, penalty=EXPONENTIAL, tau=1.5,
                                    boxes=True)
    print("records on the large grid", len(got[0]))
    assert len(got[0]) >= 1
    _same(got, detect_all_ref(scores, pairs, boxes, grid, INF, 4096, 300))


def test_exits_taken_and_not_taken(built_pair, ragged):
    """At the lowest threshold of the data nearly every wave is over the bound after its first block and leaves; at +inf no
    bound is finite and none does.  Both equal the referee, and the low threshold's list is the shorter one: a threshold that
    is ignored fails here."""
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    grid = GRIDS[2]
    scores, pairs = _planes(dev, tset, grid, CS7, piv, DEFAULT, 1.0)
    boxes = footprints(tmpls, CS7, piv).reshape(-1, 4)
    call = lambda ms: dev.exhaustive_detect_all(tset, grid, CS7, piv, max_score=ms, max_detections=256, overlap_permille=300,
                                                penalty=DEFAULT, boxes=True)
    L = call(INF)
    _same(L, detect_all_ref(scores, pairs, boxes, grid, INF, 256, 300, len(CS7), CS7, piv))
    low = f32(L[0]["score"][0])
    got = call(low)
    print("records at +inf", len(L[0]), "at the lowest score", len(got[0]), "points under it", int((scores <= low).sum()), "of",
          int((~np.isnan(scores)).sum()))
    _same(got, detect_all_ref(scores, pairs, boxes, grid, low, 256, 300, len(CS7), CS7, piv))
    assert 1 <= len(got[0]) < len(L[0]) and np.all(got[0]["score"] <= low)
    assert (scores <= low).sum() < 0.01 * (~np.isnan(scores)).sum()  # the threshold is selective: most of the plane is far


def test_special_values():
    """A volume with +inf in a region and one NaN pixel: a point whose sum meets the NaN (or inf - inf) never appears, a
    point with q = inf appears only at max_score = +inf."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    rng = np.random.default_rng(3)
    vol = np.cumsum(rng.uniform(0, 2, (2, 48, 56)).astype(np.float32), axis=2).astype(np.float32)
    vol[:, 10:22, 30:44] = np.inf
    vol[0, 35, 12] = np.nan
    dev = DeviceFeatureMap.from_volume(np.float32([0.0, 1.5]), vol, (0.0, 0.0))
    tmpls = [np.array([[0, 0, 9, 0], [0, 3, 9, 3], [2, 0, 2, 7]], dtype=np.float32).T.copy(),
             np.array([[0, 0, 0, 5]] + [[i, i % 3, i + 4, i % 3] for i in range(11)], dtype=np.float32).T.copy(),
             np.zeros((4, 0), dtype=np.float32)]
    tset = DeviceTemplates(tmpls)
    grid = dev.exhaustive_window(tset, 1, 1).as_tuple()
    scores, pairs = _planes(dev, tset, grid, None, None, DEFAULT, 1.0)
    boxes = footprints(tmpls).reshape(-1, 4)
    n_inf, n_fin = int(np.isinf(scores).sum()), int(np.isfinite(scores).sum())
    assert n_inf > 0 and n_fin > 0 and np.isnan(scores).sum() > 0  # all three kinds of point occur
    ms = f32(np.median(scores[np.isfinite(scores)]))
    for permille, md in [(1000, 4096), (300, 64)]:
        for thr in (ms, f32(np.finfo(np.float32).max), INF):
            got = dev.exhaustive_detect_all(tset, grid, max_score=thr, max_detections=md, overlap_permille=permille, penalty=DEFAULT,
                                            boxes=True)
            _same(got, detect_all_ref(scores, pairs, boxes, grid, thr, md, permille))
            assert not np.isnan(got[0]["score"]).any() and (thr == INF or not np.isinf(got[0]["score"]).any())
            if permille == 1000:  # nothing suppressed: every point under the threshold, and no other
                with np.errstate(invalid="ignore"):
                    assert len(got[0]) == int((scores <= thr).sum())
    every = dev.exhaustive_detect_all(tset, grid, max_score=INF, max_detections=4096, overlap_permille=1000, penalty=DEFAULT)
    assert len(every) == n_inf + n_fin and np.isinf(every["score"]).sum() == n_inf


def test_capped_set(built_pair, ragged):
    """A set with line_caps = 3.0 against the referee on its own capped planes (the clamping form of the kernel)."""
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    tmpls, _, piv = ragged
    capped = DeviceTemplates(tmpls, line_caps=3.0)
    grid = GRIDS[0]
    scores, pairs = _planes(dev, capped, grid, CS7, piv, DEFAULT, 1.0)
    boxes = footprints(tmpls, CS7, piv, 2).reshape(-1, 4)
    call = lambda ms: dev.exhaustive_detect_all(capped, grid, CS7, piv, max_score=ms, max_detections=128, overlap_permille=300, margin=2,
                                                penalty=DEFAULT, boxes=True)
    L = call(INF)
    _same(L, detect_all_ref(scores, pairs, boxes, grid, INF, 128, 300, len(CS7), CS7, piv))
    for ms in _thresholds(L[0]):
        _same(call(ms), detect_all_ref(scores, pairs, boxes, grid, ms, 128, 300, len(CS7), CS7, piv))
    assert len(call(f32(L[0]["score"][0]))[0]) < len(L[0])


def test_all_zero_volume_ties():
    """Every q is 0: with max_score = 0 every point passes and the list is the lattice test_all_zero_volume_ties of the
    overlap call predicts, here past 64 records."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    dev = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 40, 30), dtype=np.float32), (0.0, 0.0))
    tmpls = [np.array([[2, 3, 10, 12], [5, 5, 6, 20]], dtype=np.float32).T.copy(), np.array([[1, 1, 2, 2]], dtype=np.float32).T.copy()]
    tset = DeviceTemplates(tmpls)
    grid = (-5, -4, 37, 29, 1, 1)
    boxes = footprints(tmpls).reshape(-1, 4)
    scores, pairs = _planes(dev, tset, grid, None, None, None, 1.0)
    assert np.all(scores[pairs >= 0] == 0)
    for permille in (0, 300, 1000):
        for md in (7, 64, 500):
            want = detect_all_ref(scores, pairs, boxes, grid, 0.0, md, permille)
            _same(dev.exhaustive_detect_all(tset, grid, max_score=0.0, max_detections=md, overlap_permille=permille, boxes=True), want)
            _same(dev.exhaustive_detect_all(tset, grid, max_score=INF, max_detections=md, overlap_permille=permille, boxes=True), want)
    rec = dev.exhaustive_detect_all(tset, grid, max_score=0.0, max_detections=4096, overlap_permille=1000)
    assert len(rec) == int((pairs >= 0).sum()) > 64 and np.all(rec["score"] == 0)
    g = ((rec["transform"][:, 5] - grid[1]) * grid[2] + (rec["transform"][:, 2] - grid[0])).astype(np.int64)
    assert np.array_equal(g, np.flatnonzero(pairs.reshape(-1) >= 0))  # pure grid order
    lattice = dev.exhaustive_detect_all(tset, grid, max_score=0.0, max_detections=64, overlap_permille=0, boxes=True)
    nms = dev.exhaustive_detect_nms(tset, grid, k=64, overlap_permille=0, boxes=True)
    assert lattice[0].tobytes() == nms[0].tobytes() and np.array_equal(lattice[1], nms[1]) and len(nms[0]) > 2


def test_degenerate_inputs(built_pair, ragged):
    """A far grid, a set whose only template has no lines, a 1 x 1 grid."""
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    far = (5000, 5000, 40, 30, 1, 1)
    rec, box = dev.exhaustive_detect_all(tset, far, CS7, piv, max_score=INF, max_detections=100, boxes=True)
    assert len(rec) == 0 and box.shape == (0, 4)
    assert len(dev.exhaustive_detect_all(tset, far, max_score=1.0)) == 0
    none = DeviceTemplates([np.zeros((4, 0), dtype=np.float32)])
    rec, box = dev.exhaustive_detect_all(none, GRIDS[0], max_score=INF, boxes=True)
    assert len(rec) == 0 and box.shape == (0, 4)
    assert len(dev.exhaustive_detect_all(DeviceTemplates([]), GRIDS[0], max_score=INF)) == 0
    x0, y0, nx, ny, _, _ = GRIDS[0]
    scores, pairs = _planes(dev, tset, GRIDS[0], None, None, DEFAULT, 1.0)
    cand = np.argwhere(pairs >= 0)
    j, i = cand[np.argmin(np.abs(cand - [ny // 2, nx // 2]).sum(axis=1))]
    one = (x0 + int(i), y0 + int(j), 1, 1, 1, 1)
    s = scores[j, i]
    boxes = footprints(tmpls).reshape(-1, 4)
    p1 = _planes(dev, tset, one, None, None, DEFAULT, 1.0)
    assert p1[0][0, 0] == s
    assert s > 0
    for ms, n in [(INF, 1), (s, 1), (np.nextafter(s, f32(0)), 0)]:
        got = dev.exhaustive_detect_all(tset, one, max_score=ms, max_detections=5, penalty=DEFAULT, boxes=True)
        assert len(got[0]) == n
        _same(got, detect_all_ref(p1[0], p1[1], boxes, one, ms, 5, 300))


def test_repeatability_and_public_api(built_pair, ragged):
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    call = lambda base=0: dev.exhaustive_detect_all(tset, GRIDS[1], CS7, piv, max_score=INF, max_detections=150, overlap_permille=500,
                                                    margin=1, penalty=EXPONENTIAL, tau=1.5, tmpl_index_base=base, boxes=True)
    first = call()
    assert len(first[0]) > 64
    ms = first[0]["score"][70]
    low = lambda: dev.exhaustive_detect_all(tset, GRIDS[1], CS7, piv, max_score=ms, max_detections=150, overlap_permille=500, margin=1,
                                            penalty=EXPONENTIAL, tau=1.5, boxes=True)
    l1 = low()
    for _ in range(2):
        again, l2 = call(), low()
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
        assert l2[0].tobytes() == l1[0].tobytes() and l2[1].tobytes() == l1[1].tobytes()
    shifted = call(-7)
    assert np.array_equal(shifted[0]["tmpl_idx"], first[0]["tmpl_idx"] - 7) and np.array_equal(shifted[1], first[1])

    import openfdcm_amd as fd
    img = np.full((160, 200), 40, dtype=np.uint8)
    img[30:70, 25:85] = 200
    img[90:140, 120:150] = 200
    box = lambda w, h: np.array([(0, 0, w, 0), (w, 0, w, h), (w, h, 0, h), (0, h, 0, 0)], dtype=np.float32).T.copy()
    shapes = [box(58, 38), np.zeros((4, 0), dtype=np.float32), box(28, 48), box(40, 40)]
    dt3 = fd.build_image_featuremap(img, fd.Dt3CpuParameters(depth=12, dt3Coeff=5.0, distance=fd.L2), threshold=60)
    pen = fd.ExponentialPenalty(1.5)
    every, boxes = fd.exhaustive_detect_all(dt3, shapes, np.inf, overlap=0.3, max_detections=64, penalty=pen, margin=2, return_boxes=True)
    nms, nboxes = fd.exhaustive_detect_nms(dt3, shapes, overlap=0.3, k=64, penalty=pen, margin=2, return_boxes=True)
    assert isinstance(every, fd.MatchList) and boxes.shape == (len(every), 4) and boxes.dtype == np.int32
    assert every.records().tobytes() == nms.records().tobytes() and np.array_equal(boxes, nboxes)
    ms = every[1].score  # the two drawn boxes are the two best: a threshold at the second returns them and nothing else
    two, b2 = fd.exhaustive_detect_all(dt3, shapes, ms, overlap=0.3, penalty=pen, margin=2, return_boxes=True)
    assert isinstance(two, fd.MatchList) and b2.shape == (len(two), 4)
    assert two.records().tobytes() == every.records()[:len(two)].tobytes() and 2 <= len(two) < len(every)
    assert sorted(two.records()["tmpl_idx"][:2]) == [0, 2]
    assert isinstance(fd.exhaustive_detect_all(dt3, shapes, 0.0), fd.MatchList)
    angled = fd.exhaustive_detect_all(dt3, shapes, ms, stride=2, angles=np.deg2rad([0, 90]), penalty=pen)
    assert isinstance(angled, fd.MatchList) and all(angled[i].score <= ms for i in range(len(angled)))
    b = fd.detect_score_bounds(shapes, pen, ms)
    assert b.shape == (4,) and b[1] == 0 and np.all(b[[0, 2, 3]] > 0)
    with pytest.raises(fd._capi.FdcmError):
        fd.exhaustive_detect_all(dt3, shapes, -1.0)
    with pytest.raises(fd._capi.FdcmError):
        fd.exhaustive_detect_all(dt3, shapes, 1.0, max_detections=5000)
    wide = np.array([[-400.0, 0.0, dt3._fm.width + 400.0, 0.0]], dtype=np.float32).T.copy()
    m3, b3 = fd.exhaustive_detect_all(dt3._fm, [wide], 1.0, return_boxes=True)
    assert len(m3) == 0 and b3.shape == (0, 4)
    del dt3
    fd.clear_featuremap_pool()
