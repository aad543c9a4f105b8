"""GPU tests of the best map and the detections (include/fdcm.h, "Best map and detections"): both planes and the records
against the numpy definition (detect_ref.py) applied to the device's and to the oracle's score volumes, one template
against fdcm_search_exhaustive_peaks, ties on an all-zero volume, a known answer with two planted templates, order
independence, the limits that need handles, and the public Python surface on an image-built feature map."""
import ctypes as C

import numpy as np
import pytest

from detect_ref import best_ref, detect_ref, normalised, records
from oracle import oracle as O
from peaks_ref import peak_mask, peaks
from test_gpu_exhaustive import SIZES, _grid_points, _same_bits, _templates_with_sizes
from test_gpu_exhaustive_peaks import GRIDS

pytestmark = pytest.mark.gpu

DEFAULT, EXPONENTIAL = 0, 1
PENALTIES = [(None, 1.0), (DEFAULT, 1.0), (EXPONENTIAL, 1.5)]
RADII = [(0, 0), (1, 1), (3, 1), (0, 5), (8, 8), (32, 32)]


def _cs(deg):
    a = np.deg2rad(np.asarray(deg, dtype=np.float64))
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)


def _centers(tmpls):
    out = np.zeros((len(tmpls), 2), dtype=np.float32)
    for t, tm in enumerate(tmpls):
        if tm.shape[1]:
            xs, ys = np.concatenate([tm[0], tm[2]]), np.concatenate([tm[1], tm[3]])
            out[t] = [(xs.min() + xs.max()) / np.float32(2), (ys.min() + ys.max()) / np.float32(2)]
    return out


CS7 = _cs([0, 20, 45, 90, 135, 250, 330])
ROTS = {"none": None, "seven": CS7, "one": np.float32([[1, 0]])}


@pytest.fixture(scope="module")
def built_pair():
    from openfdcm_amd import synthetic
    from openfdcm_amd.engine import DeviceFeatureMap
    scene = synthetic.scene(256, 48, 9)
    dev = DeviceFeatureMap.build(scene, depth=12, coeff=5.0, padding=1.2, distance=0)
    orc = O.build(scene, depth=12, coeff=5.0, padding=1.2, distance=O.L2, nthreads=8)
    return scene, dev, orc


@pytest.fixture(scope="module")
def ragged(built_pair):
    """24 templates of 0 (the first: no lines) to 40 lines: three chunks of the scoring kernel meet at every point."""
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    rng = np.random.default_rng(23)
    tmpls = _templates_with_sizes(rng, dev.width / 1.2, SIZES)
    return tmpls, DeviceTemplates(tmpls), _centers(tmpls)


@pytest.fixture(scope="module")
def volumes(built_pair, ragged):
    """The device's score volumes (T, A, ny, nx) of the ragged set, computed once per (rotations, grid) and left unchanged."""
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    cache = {}

    def get(rot, grid):
        if (rot, grid) not in cache:
            cs = ROTS[rot]
            v = dev.score_map(tset, grid)[:, None] if cs is None else dev.rotation_score_map(tset, grid, cs, piv)
            v.setflags(write=False)
            cache[(rot, grid)] = v
        return cache[(rot, grid)]
    return get


def _same_records(got, want):
    assert len(got) == len(want)
    assert np.array_equal(got["tmpl_idx"], want["tmpl_idx"])
    assert _same_bits(got["score"], want["score"])
    assert got.tobytes() == want.tobytes()


def _same_planes(got, want):
    assert np.array_equal(got[1], want[1])
    assert got[0].dtype == np.float32 and got[0].tobytes() == want[0].tobytes()  # NaN is the one quiet NaN


@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[1]])
@pytest.mark.parametrize("rot", ["none", "seven", "one"])
@pytest.mark.parametrize("penalty,tau", PENALTIES)
def test_best_map_against_the_definition(built_pair, ragged, volumes, grid, rot, penalty, tau):
    """Both planes equal detect_ref on the device's own score volume of the same grid, bit for bit.  The inputs are no
    degenerate case (checked beforehand on the oracle's scores): points without candidates, at least 5 winning templates
    and, over the seven angles, at least 3 winning angles."""
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    cs = ROTS[rot]
    q = normalised(volumes(rot, grid), tset.lengths(), penalty, tau)
    want = best_ref(q, skip={0})
    got = dev.best_map(tset, grid, cs, None if cs is None else piv, penalty=penalty, tau=tau)
    _same_planes(got, want)
    pairs = got[1]
    A = q.shape[1]
    assert (pairs < 0).sum() > 1000 and (pairs >= 0).sum() > 10000
    assert len(np.unique(pairs[pairs >= 0] // A)) >= 5 and 0 not in pairs[pairs >= 0] // A
    if rot == "seven":
        assert len(np.unique(pairs[pairs >= 0] % A)) >= 3


def test_best_map_of_the_large_grid(built_pair, ragged, volumes):
    """467 x 459: many sub-tiles per workgroup, the grid wider and taller than every box."""
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    grid = GRIDS[2]
    q = normalised(volumes("none", grid), tset.lengths(), EXPONENTIAL, 1.5)
    _same_planes(dev.best_map(tset, grid, penalty=EXPONENTIAL, tau=1.5), best_ref(q, skip={0}))
    for rx, ry in [(3, 1), (32, 32)]:
        _same_records(dev.exhaustive_detect(tset, grid, k=64, rx=rx, ry=ry, penalty=EXPONENTIAL, tau=1.5),
                      detect_ref(q, 64, rx, ry, grid, skip={0}))


@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[1]])
@pytest.mark.parametrize("rot,penalty,tau", [("none", None, 1.0), ("seven", EXPONENTIAL, 1.5), ("one", DEFAULT, 1.0)])
def test_detections_against_the_definition(built_pair, ragged, volumes, grid, rot, penalty, tau):
    """The records equal detect_ref byte for byte at every radius and k; more than one detection exists at every radius."""
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    cs = ROTS[rot]
    pv = None if cs is None else piv
    q = normalised(volumes(rot, grid), tset.lengths(), penalty, tau)
    scores, pairs = best_ref(q, skip={0})  # once: detect_ref is the peaks of this plane with the poses of its pairs
    for rx, ry in RADII:
        assert peak_mask(scores, rx, ry).sum() > 1
        for k in (1, 8, 64):
            got = dev.exhaustive_detect(tset, grid, cs, pv, k=k, rx=rx, ry=ry, penalty=penalty, tau=tau)
            g, s = peaks(scores, k, rx, ry)
            _same_records(got, records(g, s, pairs, q.shape[1], cs, pv, grid))
    got = dev.exhaustive_detect(tset, grid, cs, pv, k=8, rx=3, ry=1, penalty=penalty, tau=tau, tmpl_index_base=-7)
    _same_records(got, detect_ref(q, 8, 3, 1, grid, cs=cs, pivots=pv, base=-7, skip={0}))
    assert np.all(np.diff(got["score"]) >= 0)


def test_detections_of_the_oracle_volume(built_pair, ragged):
    """The chain does not rest on the device alone: the volume the referee judges is the oracle's evaluate<Dt3Cpu> at every
    admissible point (NaN where the seam says so), for four templates."""
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    tmpls, _, _ = ragged
    sub = [tmpls[t] for t in (3, 9, 17, 23)]
    tset = DeviceTemplates(sub)
    grid = GRIDS[0]
    nan = np.isnan(dev.score_map(tset, grid))
    pts = _grid_points(grid).reshape(-1, 2)
    maps = np.full(nan.shape, np.nan, dtype=np.float32)
    for t, tm in enumerate(sub):
        adm = ~nan[t].reshape(-1)
        flat = maps[t].reshape(-1)
        flat[adm] = O.evaluate(orc, tm, pts[adm])
        maps[t] = flat.reshape(maps[t].shape)
    assert (~nan).sum() > 5000
    for penalty, tau in PENALTIES:
        q = normalised(maps[:, None], tset.lengths(), penalty, tau)
        _same_planes(dev.best_map(tset, grid, penalty=penalty, tau=tau), best_ref(q))
        for rx, ry in [(1, 1), (3, 1), (8, 8)]:
            _same_records(dev.exhaustive_detect(tset, grid, k=16, rx=rx, ry=ry, penalty=penalty, tau=tau),
                          detect_ref(q, 16, rx, ry, grid))


@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[1]])
def test_one_template_is_the_peaks_call(built_pair, ragged, grid):
    """One template, no penalty, no rotations: the records are fdcm_search_exhaustive_peaks', byte for byte, and the score
    plane is fdcm_score_map's."""
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    tmpls, _, _ = ragged
    tset = DeviceTemplates([tmpls[17]])
    scores, pairs = dev.best_map(tset, grid)
    plane = dev.score_map(tset, grid)[0]
    assert scores.tobytes() == plane.tobytes() and np.array_equal(pairs, np.where(np.isnan(plane), -1, 0))
    for (rx, ry), k in zip(RADII, (1, 8, 64, 8, 64, 8)):
        want = dev.exhaustive_peaks(tset, grid, k=k, rx=rx, ry=ry, tmpl_index_base=5)
        assert len(want) > 0
        assert dev.exhaustive_detect(tset, grid, k=k, rx=rx, ry=ry, tmpl_index_base=5).tobytes() == want.tobytes()


def test_all_zero_volume_ties():
    """Every score is 0, with three templates of which the last is a copy of the first: every candidate point names the
    lowest admissible template (and angle), and the detections follow the lowest-grid-index rule."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    dev = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 40, 30), dtype=np.float32), (0.0, 0.0))
    a = np.array([[2, 3, 10, 12], [5, 5, 6, 20]], dtype=np.float32).T.copy()
    tmpls = [a, np.array([[1, 1, 2, 2]], dtype=np.float32).T.copy(), a.copy()]
    tset = DeviceTemplates(tmpls)
    grid = (-25, -24, 60, 61, 1, 1)
    cs = _cs([30, 0, 90])
    piv = _centers(tmpls)
    for c, pv in [(None, None), (cs, piv)]:
        vol = dev.score_map(tset, grid)[:, None] if c is None else dev.rotation_score_map(tset, grid, c, pv)
        A = vol.shape[1]
        adm = ~np.isnan(vol).reshape(3 * A, grid[3], grid[2])
        lowest = np.where(adm.any(axis=0), adm.argmax(axis=0), -1)
        assert set(np.unique(lowest)) >= {-1, 0, A} and 2 * A not in lowest  # the copy never wins: template 0 does
        for penalty, tau in PENALTIES:
            scores, pairs = dev.best_map(tset, grid, c, pv, penalty=penalty, tau=tau)
            assert np.array_equal(pairs, lowest)
            assert np.all(scores[lowest >= 0] == 0) and np.isnan(scores[lowest < 0]).all()
            q = normalised(vol, tset.lengths(), penalty, tau)
            for (rx, ry) in [(0, 0), (1, 1), (0, 2), (3, 0), (32, 32)]:
                for k in (1, 7, 64):
                    got = dev.exhaustive_detect(tset, grid, c, pv, k=k, rx=rx, ry=ry, penalty=penalty, tau=tau)
                    _same_records(got, detect_ref(q, k, rx, ry, grid, cs=c, pivots=pv))
        # radius 0: the first k candidate points in grid order
        got = dev.exhaustive_detect(tset, grid, c, pv, k=64)
        g = np.flatnonzero(lowest.reshape(-1) >= 0)[:64]
        assert np.array_equal(got["tmpl_idx"], lowest.reshape(-1)[g] // A)


def test_known_answer_two_templates():
    """Two shapes planted in a scene, one as it is and one turned by 90 degrees, among templates that resemble them: the
    two best detections are score 0 and name the exact templates, their angles and their translations, and no template
    gives a further detection within the radius of either."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    S, r = 256, 8
    shape_a = np.array([(0, 0, 40, 0), (40, 0, 40, 30), (0, 0, 0, 45), (0, 45, 25, 45)], dtype=np.float32)
    shape_b = np.array([(0, 0, 50, 0), (50, 0, 20, 30), (20, 30, 0, 30), (0, 30, 0, 0), (10, 10, 25, 10)], dtype=np.float32)

    def variant(shape, d):
        v = shape.copy()
        v[1:, 2:] += d
        return v
    cs = np.array([[1, 0], [0, 1], [-1, 0], [0, -1]], dtype=np.float32)
    PA, PB = (30, 40), (200, 150)  # translations of shape a (angle 0) and of shape b (angle 1, pivot: the origin)
    segs = [(0, 0, S / 8, 0), (S - 1, S - 1, S - 1 - S / 8, S - 1)]
    segs += [(x1 + PA[0], y1 + PA[1], x2 + PA[0], y2 + PA[1]) for x1, y1, x2, y2 in shape_a]
    segs += [(-y1 + PB[0], x1 + PB[1], -y2 + PB[0], x2 + PB[1]) for x1, y1, x2, y2 in shape_b]
    scene = np.array(segs, dtype=np.float32).T.copy()
    dev = DeviceFeatureMap.build(scene, depth=12, coeff=5.0, padding=1.0, distance=0)
    tmpls = [variant(shape_a, 6).T.copy(), variant(shape_b, -5).T.copy(), shape_a.T.copy(), np.zeros((4, 0), dtype=np.float32),
             shape_b.T.copy(), variant(shape_a, -4).T.copy()]
    tset = DeviceTemplates(tmpls)
    grid = dev.exhaustive_rotations_window(tset, cs, None, 1, 1).as_tuple()
    vol = dev.rotation_score_map(tset, grid, cs, None)
    for penalty, tau in PENALTIES:
        got = dev.exhaustive_detect(tset, grid, cs, None, k=8, rx=r, ry=r, penalty=penalty, tau=tau)
        _same_records(got, detect_ref(normalised(vol, tset.lengths(), penalty, tau), 8, r, r, grid, cs=cs, skip={3}))
        assert len(got) > 2 and np.all(got["score"][:2] == 0) and got["score"][2] > 0
        assert got["tmpl_idx"][:2].tolist() == [2, 4]
        ta, tb = got["transform"][0], got["transform"][1]
        assert ta[0] == 1 and ta[3] == 0 and abs(ta[2] - PA[0]) <= 2 and abs(ta[5] - PA[1]) <= 2
        assert tb[0] == 0 and tb[3] == 1 and abs(tb[2] - PB[0]) <= 2 and abs(tb[5] - PB[1]) <= 2
        for t in got["transform"][2:]:  # the variants peak at the same places in their own maps: no detection there
            for p in (ta, tb):
                assert abs(t[2] - p[2]) > r or abs(t[5] - p[5]) > r


def test_order_independence(built_pair, ragged, volumes):
    """The same call twice gives the same bytes.  With the template list reversed the score plane is the same and the pair
    plane names the same (template, angle) wherever one template alone has the lowest score."""
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    grid = GRIDS[0]
    T, A = len(tmpls), len(CS7)
    first = dev.best_map(tset, grid, CS7, piv, penalty=EXPONENTIAL, tau=1.5)
    again = dev.best_map(tset, grid, CS7, piv, penalty=EXPONENTIAL, tau=1.5)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    d1 = dev.exhaustive_detect(tset, grid, CS7, piv, k=64, rx=3, ry=1, penalty=EXPONENTIAL, tau=1.5)
    assert dev.exhaustive_detect(tset, grid, CS7, piv, k=64, rx=3, ry=1, penalty=EXPONENTIAL, tau=1.5).tobytes() == d1.tobytes()
    rev = DeviceTemplates(tmpls[::-1])
    rs, rp = dev.best_map(rev, grid, CS7, piv[::-1].copy(), penalty=EXPONENTIAL, tau=1.5)
    assert rs.tobytes() == first[0].tobytes()
    assert np.array_equal(rp < 0, first[1] < 0)
    back = np.where(rp >= 0, (T - 1 - rp // A) * A + rp % A, -1)
    q = normalised(volumes("seven", grid), tset.lengths(), EXPONENTIAL, 1.5)
    per_t = np.where(np.isnan(q), np.inf, q).min(axis=1)  # (T, ny, nx): each template's lowest q
    per_t[0] = np.inf
    alone = (per_t == per_t.min(axis=0)).sum(axis=0) == 1
    assert alone.sum() > 10000
    assert np.array_equal(back[alone & (rp >= 0)], first[1][alone & (rp >= 0)])


def test_empty_inputs_and_bad_arguments(built_pair, ragged):
    """An empty feature map, an empty template list and a set without lines give no records and planes of NaN / -1; the
    limits that need handles (T n, pivots) are FDCM_EINVAL, and a valid call afterwards is unchanged."""
    from openfdcm_amd import _capi as capi
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates, _rotations
    scene, dev, orc = built_pair
    tmpls, tset, piv = ragged
    empty = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    grid = (0, 0, 5, 4, 1, 1)
    no_lines = np.zeros((4, 0), dtype=np.float32)
    for fm, ts in [(empty, DeviceTemplates([tmpls[3]])), (dev, DeviceTemplates([])), (dev, DeviceTemplates([no_lines, no_lines]))]:
        for cs in (None, CS7[:2]):
            assert len(fm.exhaustive_detect(ts, grid, cs, k=3, rx=1, ry=1, penalty=DEFAULT)) == 0
            scores, pairs = fm.best_map(ts, grid, cs)
            assert scores.shape == (4, 5) and np.isnan(scores).all() and np.all(pairs == -1)
            assert scores.tobytes() == np.full(20, np.nan, dtype=np.float32).tobytes()
    good = (-60, -60, 50, 40, 2, 2)
    want = dev.exhaustive_detect(tset, good, CS7, piv, k=3, rx=2, ry=2, penalty=EXPONENTIAL, tau=1.5)
    assert len(want) > 0
    many = DeviceTemplates([no_lines] * (1 << 16))  # T n = 2^31
    bad_piv = piv.copy()
    bad_piv[3, 1] = np.nan
    g = capi.Grid(*good)
    out, n = C.c_void_p(), C.c_int64()
    s, p = np.zeros((40, 50), dtype=np.float32), np.zeros((40, 50), dtype=np.int32)
    for ts, cs, pv, what in [(many, np.tile(np.float32([1, 0]), (1 << 15, 1)), None, "2^31 - 1"), (tset, CS7, bad_piv, "pivots")]:
        rot, keep = _rotations(cs, pv, ts.count)
        assert capi.lib().fdcm_search_exhaustive_detect(dev._h, ts._h, C.byref(rot), C.byref(g), 3, 2, 2, -1, 1.0, 0, C.byref(out),
                                                        C.byref(n)) == -1
        assert what in capi.lib().fdcm_last_error().decode()
        assert capi.lib().fdcm_best_map(dev._h, ts._h, C.byref(rot), C.byref(g), -1, 1.0, capi.fptr(s),
                                        p.ctypes.data_as(C.POINTER(C.c_int32))) == -1
        assert what in capi.lib().fdcm_last_error().decode()
    assert dev.exhaustive_detect(tset, good, CS7, piv, k=3, rx=2, ry=2, penalty=EXPONENTIAL, tau=1.5).tobytes() == want.tobytes()
    # either plane alone
    both = dev.best_map(tset, good, CS7, piv)
    rot, keep = _rotations(CS7, piv, tset.count)
    assert capi.lib().fdcm_best_map(dev._h, tset._h, C.byref(rot), C.byref(g), -1, 1.0, capi.fptr(s), None) == 0
    assert capi.lib().fdcm_best_map(dev._h, tset._h, C.byref(rot), C.byref(g), -1, 1.0, None, p.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    assert s.tobytes() == both[0].tobytes() and np.array_equal(p, both[1])


def test_public_api():
    """openfdcm.exhaustive_detect and best_score_map on a feature map built from an image: a MatchList in ascending score
    that equals the engine call on the default window."""
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceTemplates
    img = np.full((160, 200), 40, dtype=np.uint8)
    img[30:70, 25:85] = 200   # a 60 x 40 box
    img[90:140, 120:150] = 200  # a 30 x 50 box
    box = lambda w, h: np.array([(0, 0, w, 0), (w, 0, w, h), (w, h, 0, h), (0, h, 0, 0)], dtype=np.float32).T.copy()
    tmpls = [box(58, 38), np.zeros((4, 0), dtype=np.float32), box(28, 48), box(40, 40)]
    dt3 = fd.build_image_featuremap(img, fd.Dt3CpuParameters(depth=12, dt3Coeff=5.0, distance=fd.L2), threshold=60)
    dev, tset = dt3._fm, DeviceTemplates(tmpls)
    angles = np.deg2rad([0, 90])
    cs, piv = _cs([0, 90]), _centers(tmpls)
    for penalty, kind, tau in [(None, None, 1.0), (fd.DefaultPenalty(), DEFAULT, 1.0), (fd.ExponentialPenalty(1.5), EXPONENTIAL, 1.5),
                               (fd.PenaltyStrategy(fd.ExponentialPenalty(0.5)), EXPONENTIAL, 0.5)]:
        m = fd.exhaustive_detect(dt3, tmpls, radius=8, k=6, penalty=penalty)
        assert isinstance(m, fd.MatchList) and len(m) >= 2
        assert all(m[i].score <= m[i + 1].score for i in range(len(m) - 1))
        g = fd.exhaustive_window(dt3, tmpls)
        assert m.records().tobytes() == dev.exhaustive_detect(tset, g, k=6, rx=8, ry=8, penalty=kind, tau=tau).tobytes()
        scores, pairs, g2 = fd.best_score_map(dt3, tmpls, penalty=penalty)
        raw = dev.best_map(tset, g, penalty=kind, tau=tau)
        assert g2 == g and scores.tobytes() == raw[0].tobytes() and np.array_equal(pairs, raw[1])
        # the two boxes are the two best detections, each by its own template, near where it was drawn
        rec = m.records()
        assert sorted(rec["tmpl_idx"][:2]) == [0, 2]
        for r in rec[:2]:
            want = (25, 30) if r["tmpl_idx"] == 0 else (120, 90)
            assert abs(r["transform"][2] - want[0]) <= 3 and abs(r["transform"][5] - want[1]) <= 3
    m = fd.exhaustive_detect(dt3, tmpls, radius=(6, 4), stride=2, k=5, penalty=fd.ExponentialPenalty(1.5), angles=angles)
    g = fd.rotation_window(dt3, tmpls, angles, stride=2)
    assert m.records().tobytes() == dev.exhaustive_detect(tset, g, cs, piv, k=5, rx=6, ry=4, penalty=EXPONENTIAL, tau=1.5).tobytes()
    scores, pairs, g2 = fd.best_score_map(dt3, tmpls, stride=2, penalty=fd.ExponentialPenalty(1.5), angles=angles)
    raw = dev.best_map(tset, g, cs, piv, penalty=EXPONENTIAL, tau=1.5)
    assert g2 == g and scores.tobytes() == raw[0].tobytes() and np.array_equal(pairs, raw[1])
    assert set(np.unique(pairs // 2)) <= {-1, 0, 2, 3}
    win = (10, 12, 40, 30, 2, 2)
    m2 = fd.exhaustive_detect(dt3, tmpls, radius=3, k=2, window=win)
    assert m2.records().tobytes() == dev.exhaustive_detect(tset, win, k=2, rx=3, ry=3).tobytes()
    with pytest.raises(TypeError):
        fd.exhaustive_detect(dt3, tmpls, radius=3, penalty=1.5)
    wide = np.array([[-400.0, 0.0, dev.width + 400.0, 0.0]], dtype=np.float32).T.copy()
    assert len(fd.exhaustive_detect(dev, [wide], radius=2)) == 0
    del dt3
    fd.clear_featuremap_pool()
