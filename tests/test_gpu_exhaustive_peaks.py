"""GPU tests of the exhaustive search's peaks (include/fdcm.h, "Peaks"): radius 0 against fdcm_search_exhaustive byte for
byte, every radius against the numpy definition (peaks_ref.py) applied to the device's and to the oracle's score maps,
ties on an all-zero volume, a known answer with two instances, config 2' at full size over several workspace batches,
a grid split into regions, and the public Python surface."""
import numpy as np
import pytest

from oracle import oracle as O
from peaks_ref import peak_mask, peaks_ref
from test_gpu_exhaustive import SIZES, _grid_points, _same_bits, _templates_with_sizes

pytestmark = pytest.mark.gpu


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
    """Templates of 0 (the first: no lines) to 40 lines; the map is 307 x 307 with scene translation 25.5."""
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    rng = np.random.default_rng(23)
    tmpls = _templates_with_sizes(rng, dev.width / 1.2, SIZES)
    return tmpls, DeviceTemplates(tmpls)


def _same_records(got, want):
    assert len(got) == len(want)
    assert np.array_equal(got["tmpl_idx"], want["tmpl_idx"])
    assert _same_bits(got["score"], want["score"])
    assert got.tobytes() == want.tobytes()


# grids that are no multiple of the 64 x 32 tile nor of the scoring kernel's 16 x 64 sub-tile, several tiles across,
# origins off zero, partly outside the templates' admissible boxes
GRIDS = [(-240, -60, 200, 120, 1, 1), (-241, -200, 160, 200, 3, 2), (-233, -229, 467, 459, 1, 1)]


@pytest.mark.parametrize("grid", [GRIDS[0], GRIDS[1]])
@pytest.mark.parametrize("k", [1, 8, 64])
def test_radius_zero_is_the_top_k(built_pair, ragged, grid, k):
    """rx = ry = 0: every admissible point is a peak, so the records are fdcm_search_exhaustive's, byte for byte."""
    scene, dev, orc = built_pair
    tmpls, tset = ragged
    want = dev.exhaustive_search(tset, grid, k=k)
    got = dev.exhaustive_peaks(tset, grid, k=k, rx=0, ry=0)
    assert len(want) > 0
    assert got.tobytes() == want.tobytes()
    got = dev.exhaustive_peaks(tset, grid, k=k, rx=0, ry=0, tmpl_index_base=-7)
    assert got.tobytes() == dev.exhaustive_search(tset, grid, k=k, tmpl_index_base=-7).tobytes()


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("r", [(1, 1), (3, 1), (0, 5), (8, 8), (32, 32)])
def test_peaks_against_the_definition(built_pair, ragged, grid, r):
    """The records equal peaks_ref applied to the device's score map of the same grid, for k = 1, 8 and 64."""
    scene, dev, orc = built_pair
    tmpls, tset = ragged
    rx, ry = r
    maps = dev.score_map(tset, grid)
    for k in (1, 8, 64):
        got = dev.exhaustive_peaks(tset, grid, k=k, rx=rx, ry=ry)
        _same_records(got, peaks_ref(maps, k, rx, ry, grid, skip={0}))
    assert max(peak_mask(maps[t], rx, ry).sum() for t in range(1, len(tmpls))) > 1


def test_peaks_of_the_oracle_map(built_pair, ragged):
    """The chain does not rest on the device alone: the map peaks_ref judges is the oracle's evaluate<Dt3Cpu> at every
    admissible point (NaN where the seam says so), for a few templates."""
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    tmpls, _ = ragged
    sub = [tmpls[t] for t in (3, 9, 17, 23)]
    tset = DeviceTemplates(sub)
    grid = GRIDS[0]
    nan = np.isnan(dev.score_map(tset, grid))
    pts = _grid_points(grid).reshape(-1, 2)
    maps = np.full(nan.shape, np.nan, dtype=np.float32)
    for q, tm in enumerate(sub):
        adm = ~nan[q].reshape(-1)
        flat = maps[q].reshape(-1)
        flat[adm] = O.evaluate(orc, tm, pts[adm])
        maps[q] = flat.reshape(maps[q].shape)
    assert (~nan).sum() > 5000
    for rx, ry in [(1, 1), (3, 1), (8, 8)]:
        _same_records(dev.exhaustive_peaks(tset, grid, k=16, rx=rx, ry=ry), peaks_ref(maps, 16, rx, ry, grid))


def test_all_zero_volume_ties():
    """Every score is 0: a point is a peak exactly when no lower grid index is admissible within the radius."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    dev = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 40, 30), dtype=np.float32), (0.0, 0.0))
    tmpls = [np.array([[2, 3, 10, 12], [5, 5, 6, 20]], dtype=np.float32).T.copy(),
             np.array([[1, 1, 2, 2]], dtype=np.float32).T.copy()]
    tset = DeviceTemplates(tmpls)
    grid = (-5, -4, 37, 29, 1, 1)
    maps = dev.score_map(tset, grid)
    for (rx, ry) in [(0, 0), (1, 1), (0, 2), (3, 0), (32, 32)]:
        for k in (1, 7, 64):
            got = dev.exhaustive_peaks(tset, grid, k=k, rx=rx, ry=ry)
            assert np.all(got["score"] == 0)
            _same_records(got, peaks_ref(maps, k, rx, ry, grid))
    # the admissible set is a box: with both radii >= 1 its first corner is the only peak
    got = dev.exhaustive_peaks(tset, grid, k=64, rx=1, ry=1)
    for t in range(2):
        jj, ii = np.nonzero(~np.isnan(maps[t]))
        r = got[got["tmpl_idx"] == t]
        assert len(r) == 1 and r[0]["transform"][2] == grid[0] + ii.min() and r[0]["transform"][5] == grid[1] + jj.min()
    # rx = 0, ry = 2: the window is a column, so the peaks are the box's first row
    got = dev.exhaustive_peaks(tset, grid, k=64, rx=0, ry=2)
    jj, ii = np.nonzero(~np.isnan(maps[1]))
    assert sorted(got[got["tmpl_idx"] == 1]["transform"][:, 5]) == [grid[1] + jj.min()] * min(64, len(set(ii)))


def test_known_answer_two_instances():
    """A scene made of one shape at two offsets more than 2 r apart, the shape as the template: the two best peaks both
    score 0, one in each instance's zero plateau (exhaustive_search of the same k need not leave the first one)."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    import openfdcm_amd as openfdcm
    S = 256
    shape = np.array([(0, 0, 40, 0), (40, 0, 40, 30), (0, 0, 0, 45), (0, 45, 25, 45)], dtype=np.float32)
    A, B = (30, 40), (150, 170)
    segs = [(0, 0, S / 8, 0), (S - 1, S - 1, S - 1 - S / 8, S - 1)]
    for dx, dy in (A, B):
        segs += [(x1 + dx, y1 + dy, x2 + dx, y2 + dy) for x1, y1, x2, y2 in shape]
    scene = np.array(segs, dtype=np.float32).T.copy()
    dev = DeviceFeatureMap.build(scene, depth=12, coeff=5.0, padding=1.0, distance=0)
    tmpl = shape.T.copy()
    tset = DeviceTemplates([tmpl])
    grid = dev.exhaustive_window(tset, 1, 1).as_tuple()
    maps = dev.score_map(tset, grid)
    x0, y0 = grid[0], grid[1]
    assert maps[0][A[1] - y0, A[0] - x0] == 0 and maps[0][B[1] - y0, B[0] - x0] == 0
    r = 8
    got = dev.exhaustive_peaks(tset, grid, k=2, rx=r, ry=r)
    _same_records(got, peaks_ref(maps, 2, r, r, grid))
    assert len(got) == 2 and np.all(got["score"] == 0)
    for c in (A, B):  # a score-0 peak on each instance's plateau
        assert sum(abs(t[2] - c[0]) <= 2 and abs(t[5] - c[1]) <= 2 for t in got["transform"]) == 1, (c, got)
    pub = openfdcm.exhaustive_peaks(dev, [tmpl], radius=r, k=2)
    assert sorted((m.transform[0][2], m.transform[1][2]) for m in pub) == sorted(
        (float(t[2]), float(t[5])) for t in got["transform"])


def test_config2p_full_size():
    """Config 2' (1024^2, depth 30, 1000 templates x 32 lines) at stride 2, r = 8, k = 8: the score planes of all templates
    take more than one workspace batch.  Every record is the oracle's score at its translation, and 50 templates'
    records equal peaks_ref on their score maps."""
    from openfdcm_amd import synthetic
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    cfg, scene, tmpls = synthetic.make_config("2p")
    dev = DeviceFeatureMap.build(scene, depth=cfg["depth"], coeff=5.0, padding=1.0, distance=cfg["distance"])
    orc = O.build(scene, depth=cfg["depth"], coeff=5.0, padding=1.0, distance=cfg["distance"], nthreads=16)
    tset = DeviceTemplates(tmpls)
    grid = dev.exhaustive_window(tset, 2, 2).as_tuple()
    assert grid[2] * grid[3] * 4 * len(tmpls) > 768 << 20
    recs = dev.exhaustive_peaks(tset, grid, k=8, rx=8, ry=8)
    assert np.all(np.diff(recs["tmpl_idx"]) >= 0) and len(recs) > 4 * len(tmpls)
    for t in range(len(tmpls)):
        r = recs[recs["tmpl_idx"] == t]
        assert 1 <= len(r) <= 8
        assert _same_bits(r["score"], O.evaluate(orc, tmpls[t], r["transform"][:, [2, 5]])), t
    sub = list(range(7, 1000, 20))
    maps = dev.score_map(DeviceTemplates([tmpls[t] for t in sub]), grid)
    want = peaks_ref(maps, 8, 8, 8, grid)
    want["tmpl_idx"] = np.asarray(sub)[want["tmpl_idx"]]
    got = recs[np.isin(recs["tmpl_idx"], sub)]
    _same_records(got, want)


def test_grid_split_into_regions(built_pair, ragged):
    """A grid of more points than one workspace plane holds is cut into regions whose planes carry a halo of the radii;
    this one puts a cut through the templates' admissible boxes.  The records equal peaks_ref on a small grid over the
    same boxes (NaN around them everywhere else)."""
    scene, dev, orc = built_pair
    tmpls, _ = ragged
    from openfdcm_amd.engine import DeviceTemplates
    tset = DeviceTemplates([tmpls[5], tmpls[12], tmpls[20]])
    rx, ry = 5, 3
    ny = 4096
    dx = (768 << 20) // 4 // (2048 + 2 * ry) - 2 * rx  # region width of the library's rule: strips of 2048 rows
    x0, y0 = -dx, -2000  # the cut at grid column dx is the translation x = 0, inside every box
    big = (x0, y0, dx + 200, ny, 1, 1)
    assert big[2] * big[3] > (768 << 20) // 4
    small = (-260, -260, 461, 520, 1, 1)  # holds every box's part with x < 200
    maps = dev.score_map(tset, small)
    xs = small[0] + np.arange(small[2])
    maps[:, :, xs >= x0 + big[2]] = np.nan  # outside the big grid
    for k in (3, 64):
        got = dev.exhaustive_peaks(tset, big, k=k, rx=rx, ry=ry)
        want = peaks_ref(maps, k, rx, ry, small)
        assert len(want) > 3
        assert np.array_equal(got["tmpl_idx"], want["tmpl_idx"])
        assert _same_bits(got["score"], want["score"])
        assert np.array_equal(got["transform"], want["transform"])


def test_public_api(built_pair):
    import openfdcm_amd as openfdcm
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    rng = np.random.default_rng(41)
    tmpls = _templates_with_sizes(rng, dev.width / 1.2, [6, 12, 0, 20])
    fm = openfdcm.build_cpu_featuremap(scene, openfdcm.Dt3CpuParameters(depth=12, dt3Coeff=5.0, padding=1.2))
    matches = openfdcm.exhaustive_peaks(fm, tmpls, radius=(4, 2), stride=(2, 3), k=5)
    assert len(matches) == 15 and sorted({m.tmpl_idx for m in matches}) == [0, 1, 3]
    for m in matches:
        tr = np.asarray(m.transform)
        assert tr.shape == (2, 3) and np.array_equal(tr[:, :2], np.eye(2))
    lengths = openfdcm.get_template_lengths(tmpls)
    ranked = openfdcm.sort_matches(openfdcm.penalize(openfdcm.ExponentialPenalty(1.5), matches, lengths))
    assert len(ranked) == 15 and all(ranked[i].score <= ranked[i + 1].score for i in range(14))
    maps, g = openfdcm.score_map(openfdcm.FeatureMap(fm), tmpls, stride=(2, 3))
    _same_records(matches.records(), peaks_ref(maps, 5, 4, 2, g, skip={2}))
    # radius 0 is exhaustive_search; an explicit window; tmpl_index_base
    assert openfdcm.exhaustive_peaks(fm, tmpls, radius=0, k=3).records().tobytes() == \
        openfdcm.exhaustive_search(fm, tmpls, k=3).records().tobytes()
    grid = (-10, -12, 40, 30, 2, 2)
    m2 = openfdcm.exhaustive_peaks(fm, tmpls, radius=3, k=2, window=grid)
    raw = dev.exhaustive_peaks(DeviceTemplates(tmpls), grid, k=2, rx=3, ry=3, tmpl_index_base=100)
    assert len(raw) and [m.tmpl_idx for m in m2] == [t - 100 for t in raw["tmpl_idx"]]
    wide = np.array([[-40.0, 0.0, dev.width + 40.0, 0.0]], dtype=np.float32).T.copy()
    assert len(openfdcm.exhaustive_peaks(dev, [wide], radius=2, k=3)) == 0


def test_empty_inputs_and_bad_arguments(built_pair, ragged):
    from openfdcm_amd import _capi as capi
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    import ctypes as C
    scene, dev, orc = built_pair
    tmpls, tset = ragged
    empty = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    grid = (0, 0, 5, 4, 1, 1)
    assert len(empty.exhaustive_peaks(DeviceTemplates([tmpls[3]]), grid, k=3, rx=1, ry=1)) == 0
    assert len(dev.exhaustive_peaks(DeviceTemplates([]), grid, k=3, rx=1, ry=1)) == 0
    good = (-20, -20, 30, 30, 2, 2)
    want = dev.exhaustive_peaks(tset, good, k=3, rx=2, ry=2)
    for k, rx, ry in [(0, 1, 1), (65, 1, 1), (3, -1, 0), (3, 0, 33)]:
        out, n = C.c_void_p(), C.c_int64()
        g = capi.Grid(*good)
        assert capi.lib().fdcm_search_exhaustive_peaks(dev._h, tset._h, C.byref(g), k, rx, ry, 0, C.byref(out),
                                                       C.byref(n)) == -1
        assert dev.exhaustive_peaks(tset, good, k=3, rx=2, ry=2).tobytes() == want.tobytes()
