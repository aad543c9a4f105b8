"""GPU tests of the exhaustive search over rotations (include/fdcm.h, "Rotations"): rotation score maps against the score
maps of the rotated line sets built on the host, one identity rotation against fdcm_search_exhaustive_peaks, ra = 0
against the per-template merge of the 2-D peaks, every radius against the numpy referee (rotation_ref.py) on the device's
and the oracle's maps, ties, a known answer at quarter turns, config 2' cut into regions and single-angle batches, and the
public Python surface."""
import numpy as np
import pytest

from oracle import oracle as O
from rotation_ref import peak_mask3, rot_matrix, rotated_set, rotation_peaks_ref
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
    """Templates of 0 (the first: no lines) to 40 lines, every fourth size."""
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    rng = np.random.default_rng(29)
    tmpls = _templates_with_sizes(rng, dev.width / 1.2, SIZES[::4])
    return tmpls, DeviceTemplates(tmpls)


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


def _same_records(got, want):
    assert len(got) == len(want)
    assert np.array_equal(got["tmpl_idx"], want["tmpl_idx"])
    assert _same_bits(got["score"], want["score"])
    assert got["transform"].tobytes() == want["transform"].tobytes()


CS = _cs([0, 20, 45, 90, 135, 180, 250, 330])
GRID = (-200, -180, 300, 290, 1, 1)  # no multiple of either kernel's tile, partly outside the boxes


def test_score_map_is_the_host_rotated_maps(built_pair, ragged):
    """Bit for bit the score maps of the line sets rotated on the host, NaN in the same places; a sample against the
    oracle's evaluate."""
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    tmpls, tset = ragged
    piv = _centers(tmpls)
    for pivots in (None, piv):
        got = dev.rotation_score_map(tset, GRID, CS, pivots)
        rs = rotated_set(tmpls, CS, pivots)
        want = dev.score_map(DeviceTemplates(rs), GRID).reshape(got.shape)
        assert _same_bits(got, want)
        assert (~np.isnan(got)).sum() > 10000
    pts = _grid_points(GRID).reshape(-1, 2)
    for t, a in [(1, 1), (3, 4), (5, 7)]:
        adm = ~np.isnan(got[t, a].reshape(-1))
        assert adm.sum() > 100
        sel = np.nonzero(adm)[0][::37]
        assert _same_bits(got[t, a].reshape(-1)[sel], O.evaluate(orc, rs[t * len(CS) + a], pts[sel]))


@pytest.mark.parametrize("k,rx,ry", [(1, 0, 0), (8, 0, 0), (5, 3, 1), (64, 8, 8), (7, 32, 2)])
def test_identity_rotation_is_the_2d_peaks(built_pair, ragged, k, rx, ry):
    scene, dev, orc = built_pair
    tmpls, tset = ragged
    want = dev.exhaustive_peaks(tset, GRID, k=k, rx=rx, ry=ry)
    assert len(want) > 0
    for pivots in (None, np.tile(np.float32([37.25, -11.5]), (len(tmpls), 1))):
        for ra, wrap in [(0, False), (3, True)]:
            got = dev.exhaustive_rotation_search(tset, GRID, [[1, 0]], pivots, k=k, rx=rx, ry=ry, ra=ra, wrap=wrap)
            assert np.array_equal(got["tmpl_idx"], want["tmpl_idx"])
            assert _same_bits(got["score"], want["score"])
            assert np.array_equal(got["transform"], want["transform"])  # as values: entry 1 is -0


def _merge_2d(recs2d, A, k, cs, pivots, grid):
    """Per template the k best of the 2-D records of its A rotated sets (templates t * A + a) by (score, a, g)."""
    from openfdcm_amd import _capi
    x0, y0, nx, ny, sx, sy = grid
    rows = []
    for r in recs2d:
        t, a = divmod(int(r["tmpl_idx"]), A)
        g = int((r["transform"][5] - y0) // sy) * nx + int((r["transform"][2] - x0) // sx)
        rows.append((t, int(np.float32(r["score"]).view(np.uint32)), a, g, r))
    rows.sort(key=lambda v: v[:4])
    out, count = [], {}
    for t, sbits, a, g, r in rows:
        if count.get(t, 0) >= k:
            continue
        count[t] = count.get(t, 0) + 1
        px, py = (0.0, 0.0) if pivots is None else pivots[t]
        M = rot_matrix(cs[a, 0], cs[a, 1], px, py)
        rec = np.zeros(1, dtype=_capi.MATCH_DTYPE)
        rec["tmpl_idx"] = t
        rec["score"] = r["score"]
        rec["transform"] = [[M[0, 0], M[0, 1], M[0, 2] + r["transform"][2], M[1, 0], M[1, 1], M[1, 2] + r["transform"][5]]]
        out.append(rec)
    return np.concatenate(out)


@pytest.mark.parametrize("k,rx,ry", [(1, 0, 0), (8, 2, 2), (16, 8, 3)])
def test_angle_radius_zero_is_the_merge_of_2d_peaks(built_pair, ragged, k, rx, ry):
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    tmpls, tset = ragged
    piv = _centers(tmpls)
    rs = DeviceTemplates(rotated_set(tmpls, CS, piv))
    want = _merge_2d(dev.exhaustive_peaks(rs, GRID, k=k, rx=rx, ry=ry), len(CS), k, CS, piv, GRID)
    got = dev.exhaustive_rotation_search(tset, GRID, CS, piv, k=k, rx=rx, ry=ry, ra=0)
    _same_records(got, want)
    got = dev.exhaustive_rotation_search(tset, GRID, CS, piv, k=k, rx=rx, ry=ry, ra=0, tmpl_index_base=-3)
    assert np.array_equal(got["tmpl_idx"], want["tmpl_idx"] - 3)


@pytest.mark.parametrize("r", [(0, 0, 0), (1, 1, 1), (8, 8, 1), (3, 0, 2), (0, 5, 4), (32, 32, 3), (2, 2, 32)])
@pytest.mark.parametrize("wrap", [False, True])
def test_against_the_referee(built_pair, ragged, r, wrap):
    scene, dev, orc = built_pair
    tmpls, tset = ragged
    rx, ry, ra = r
    piv = _centers(tmpls)
    grid = (-151, -140, 130, 150, 2, 3)
    vols = dev.rotation_score_map(tset, grid, CS, piv)
    for k in (1, 8, 64):
        got = dev.exhaustive_rotation_search(tset, grid, CS, piv, k=k, rx=rx, ry=ry, ra=ra, wrap=wrap)
        _same_records(got, rotation_peaks_ref(vols, CS, piv, k, rx, ry, ra, wrap, grid, skip={0}))


def test_referee_on_the_oracle_maps(built_pair, ragged):
    """The chain does not rest on the device alone: the volumes judged are the oracle's evaluate at every admissible point."""
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    tmpls, _ = ragged
    sub = [tmpls[2], tmpls[5]]
    tset = DeviceTemplates(sub)
    piv = _centers(sub)
    cs = CS[:5]
    grid = (-120, -100, 96, 80, 2, 2)
    nan = np.isnan(dev.rotation_score_map(tset, grid, cs, piv))
    pts = _grid_points(grid).reshape(-1, 2)
    rs = rotated_set(sub, cs, piv)
    vols = np.full(nan.shape, np.nan, dtype=np.float32)
    for t in range(len(sub)):
        for a in range(len(cs)):
            adm = ~nan[t, a].reshape(-1)
            flat = vols[t, a].reshape(-1)
            flat[adm] = O.evaluate(orc, rs[t * len(cs) + a], pts[adm])
            vols[t, a] = flat.reshape(vols[t, a].shape)
    assert (~nan).sum() > 5000
    for rx, ry, ra, wrap in [(1, 1, 1, True), (4, 2, 1, False), (8, 8, 2, True)]:
        got = dev.exhaustive_rotation_search(tset, grid, cs, piv, k=16, rx=rx, ry=ry, ra=ra, wrap=wrap)
        _same_records(got, rotation_peaks_ref(vols, cs, piv, 16, rx, ry, ra, wrap, grid))


def test_all_zero_volume_ties():
    """Every score is 0: the lowest angle wins, then the lowest grid index; with wrap angle 0 is in angle n - 1's window."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    dev = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 40, 30), dtype=np.float32), (0.0, 0.0))
    tmpls = [np.array([[2, 3, 10, 12], [5, 5, 6, 20]], dtype=np.float32).T.copy()]
    tset = DeviceTemplates(tmpls)
    cs = _cs([0, 90, 180, 270, 30])
    piv = _centers(tmpls)
    grid = (-25, -24, 30, 31, 1, 1)
    vols = dev.rotation_score_map(tset, grid, cs, piv)
    assert not np.isnan(vols[0, 0]).all() and not np.isnan(vols[0, 4]).all()
    for rx, ry, ra, wrap in [(0, 0, 0, False), (1, 1, 1, False), (0, 0, 1, True), (0, 0, 1, False), (32, 32, 32, True)]:
        for k in (1, 9, 64):
            got = dev.exhaustive_rotation_search(tset, grid, cs, piv, k=k, rx=rx, ry=ry, ra=ra, wrap=wrap)
            assert np.all(got["score"] == 0)
            _same_records(got, rotation_peaks_ref(vols, cs, piv, k, rx, ry, ra, wrap, grid))
    # the whole volume in one window: the first admissible point of angle 0 is the only peak
    got = dev.exhaustive_rotation_search(tset, grid, cs, piv, k=64, rx=32, ry=32, ra=32, wrap=True)
    jj, ii = np.nonzero(~np.isnan(vols[0, 0]))
    assert len(got) == 1 and got[0]["transform"][0] == 1
    M = rot_matrix(1, 0, *piv[0])
    assert got[0]["transform"][2] == M[0, 2] + np.float32(grid[0] + ii[jj == jj.min()].min())
    # ra = 1, rx = ry = 0: angle 4 has angle 0 in its window only with wrap, and wrap changes the answer
    assert (~np.isnan(vols[0, 0]) & ~np.isnan(vols[0, 4]) & np.isnan(vols[0, 3])).any()
    masks = [peak_mask3(vols[0], 0, 0, 1, w) for w in (False, True)]
    assert (masks[0][4] & ~masks[1][4]).any() and np.array_equal(masks[0][:4], masks[1][:4])
    # the device sees it too: angle 4 alone against angles 3, 4, 0 (its wrap neighbour) given in that order
    sub = cs[[3, 4, 0]]
    v3 = dev.rotation_score_map(tset, grid, sub, piv)
    for wrap in (False, True):
        got = dev.exhaustive_rotation_search(tset, grid, sub, piv, k=64, rx=0, ry=0, ra=1, wrap=wrap)
        _same_records(got, rotation_peaks_ref(v3, sub, piv, 64, 0, 0, 1, wrap, grid))


def test_known_answer_quarter_turns():
    """A scene holding one shape turned by 90 and by 180 degrees at integer offsets: with k = 2 and ra = 1 both placements
    come back at score 0 with their exact rotation, on their instance's zero plateau."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    S = 256
    shape = np.array([(0, 0, 40, 0), (40, 0, 40, 30), (0, 0, 0, 45), (0, 45, 25, 45)], dtype=np.float32)
    cs = np.array([[1, 0], [0, 1], [-1, 0], [0, -1]], dtype=np.float32)
    A, B = (80, 40), (200, 220)  # translations of the 90 and the 180 degree copies (pivot: the origin)
    segs = [(0, 0, S / 8, 0), (S - 1, S - 1, S - 1 - S / 8, S - 1)]
    for (c, s), (dx, dy) in (((0, 1), A), ((-1, 0), B)):
        for x1, y1, x2, y2 in shape:
            segs.append((c * x1 - s * y1 + dx, s * x1 + c * y1 + dy, c * x2 - s * y2 + dx, s * x2 + c * y2 + dy))
    scene = np.array(segs, dtype=np.float32).T.copy()
    dev = DeviceFeatureMap.build(scene, depth=12, coeff=5.0, padding=1.0, distance=0)
    tmpl = shape.T.copy()
    tset = DeviceTemplates([tmpl])
    grid = dev.exhaustive_rotations_window(tset, cs, None, 1, 1).as_tuple()
    vols = dev.rotation_score_map(tset, grid, cs, None)
    x0, y0 = grid[0], grid[1]
    assert vols[0, 1, A[1] - y0, A[0] - x0] == 0 and vols[0, 2, B[1] - y0, B[0] - x0] == 0
    got = dev.exhaustive_rotation_search(tset, grid, cs, None, k=2, rx=8, ry=8, ra=1, wrap=True)
    _same_records(got, rotation_peaks_ref(vols, cs, None, 2, 8, 8, 1, True, grid))
    assert len(got) == 2 and np.all(got["score"] == 0)
    for (c, s), (dx, dy) in (((0, 1), A), ((-1, 0), B)):
        r = [t for t in got["transform"] if t[0] == c and t[3] == s]
        assert len(r) == 1, got
        t = r[0]
        assert t[1] == -s and t[4] == c and abs(t[2] - dx) <= 2 and abs(t[5] - dy) <= 2


def test_config2p_regions_and_single_angle_batches():
    """Config 2' at stride 1 on a grid of more points than the map workspace holds with the angle halo: the grid is cut
    into regions (a row cut and a column cut through the boxes) and every batch holds 2 ra + 1 planes, so it decides one
    angle and each template's angle range is cut across batches.  The records equal the referee on a small grid over the
    same boxes (NaN everywhere else on the big one)."""
    from openfdcm_amd import synthetic
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    cfg, scene, tmpls = synthetic.make_config("2p")
    dev = DeviceFeatureMap.build(scene, depth=cfg["depth"], coeff=5.0, padding=1.0, distance=cfg["distance"])
    sub = [tmpls[3], tmpls[400]]
    tset = DeviceTemplates(sub)
    cs = _cs(np.arange(0, 360, 30))
    piv = _centers(sub)
    small = dev.exhaustive_rotations_window(tset, cs, piv, 1, 1).as_tuple()
    rx, ry, ra = 5, 3, 2
    pts = (512 << 20) // 4
    dx = pts // 5 // (2048 + 2 * ry) - 2 * rx  # region width of the library's rule, 5 = 2 ra + 1 planes
    cx, cy = small[0] + small[2] // 2, small[1] + small[3] // 2  # cuts inside the boxes
    big = (cx - dx, cy - 2048, dx + small[0] + small[2] - cx + 40, 2048 + small[1] + small[3] - cy + 40, 1, 1)
    assert big[0] <= small[0] and big[1] <= small[1] and big[2] * big[3] * 5 > pts
    vols = dev.rotation_score_map(tset, small, cs, piv)
    for k, wrap in [(3, True), (20, False)]:
        got = dev.exhaustive_rotation_search(tset, big, cs, piv, k=k, rx=rx, ry=ry, ra=ra, wrap=wrap)
        want = rotation_peaks_ref(vols, cs, piv, k, rx, ry, ra, wrap, small)
        assert len(want) >= 2 * min(k, 3)
        _same_records(got, want)


def test_config2p_topk_is_the_merge_of_the_host_rotated_top_k():
    """The benchmark's rotation case: config 2', 100 templates x 36 angles (115200 rotated lines: the host preparation
    runs in several threads), stride 2, k = 8, ra = rx = ry = 0, against the per-template merge of fdcm_search_exhaustive
    over the host-rotated line sets."""
    from openfdcm_amd import synthetic
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    cfg, scene, tmpls = synthetic.make_config("2p")
    dev = DeviceFeatureMap.build(scene, depth=cfg["depth"], coeff=5.0, padding=1.0, distance=cfg["distance"])
    sub = tmpls[:100]
    cs = _cs(np.arange(0, 360, 10))
    piv = _centers(sub)
    tset = DeviceTemplates(sub)
    grid = dev.exhaustive_rotations_window(tset, cs, piv, 2, 2).as_tuple()
    rs = DeviceTemplates(rotated_set(sub, cs, piv))
    assert grid == dev.exhaustive_window(rs, 2, 2).as_tuple()
    want = _merge_2d(dev.exhaustive_search(rs, grid, k=8), len(cs), 8, cs, piv, grid)
    got = dev.exhaustive_rotation_search(tset, grid, cs, piv, k=8, wrap=True)
    assert len(got) == 800
    _same_records(got, want)


def test_public_api(built_pair):
    import openfdcm_amd as openfdcm
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    rng = np.random.default_rng(43)
    tmpls = _templates_with_sizes(rng, dev.width / 1.2, [6, 12, 0, 20])
    angles = np.deg2rad([0, 40, 80, 120, 160, 200, 240, 280, 320])
    cs = np.stack([np.cos(angles), np.sin(angles)], axis=1).astype(np.float32)
    fm = openfdcm.build_cpu_featuremap(scene, openfdcm.Dt3CpuParameters(depth=12, dt3Coeff=5.0, padding=1.2))
    tset = DeviceTemplates(tmpls)
    # the window: brute force over the per-(t, a) boxes, i.e. the window of the rotated sets as one template set
    for pivot, pv in [("center", _centers(tmpls)), (None, None), (np.float32([[1, 2], [3, 4], [5, 6], [7, 8]]), None)]:
        pv = pivot if isinstance(pivot, np.ndarray) else pv
        for stride in (1, (2, 3)):
            win = openfdcm.rotation_window(fm, tmpls, angles, stride=stride, pivot=pivot)
            sx, sy = (stride, stride) if np.ndim(stride) == 0 else stride
            assert win == dev.exhaustive_window(DeviceTemplates(rotated_set(tmpls, cs, pv)), sx, sy).as_tuple()
        m = openfdcm.exhaustive_rotation_search(fm, tmpls, angles, stride=2, k=4, radius=(3, 2), angle_radius=1, wrap=True,
                                                pivot=pivot)
        g = openfdcm.rotation_window(fm, tmpls, angles, stride=2, pivot=pivot)
        raw = dev.exhaustive_rotation_search(tset, g, cs, pv, k=4, rx=3, ry=2, ra=1, wrap=True)
        assert m.records().tobytes() == raw.tobytes()
        maps, g2 = openfdcm.rotation_score_map(fm, tmpls, angles, stride=2, pivot=pivot)
        assert g2 == g and maps.shape == (4, len(angles), g[3], g[2])
        _same_records(m.records(), rotation_peaks_ref(maps, cs, pv, 4, 3, 2, 1, True, g, skip={2}))
    assert len(m) == 12 and sorted({r.tmpl_idx for r in m}) == [0, 1, 3]
    lengths = openfdcm.get_template_lengths(tmpls)
    ranked = openfdcm.sort_matches(openfdcm.penalize(openfdcm.ExponentialPenalty(1.5), m, lengths))
    assert len(ranked) == 12 and all(ranked[i].score <= ranked[i + 1].score for i in range(11))
    tr = np.asarray(ranked[0].transform)
    assert tr.shape == (2, 3) and abs(tr[0, 0] * tr[1, 1] - tr[0, 1] * tr[1, 0] - 1) < 1e-5
    # an explicit window; every template outside the map
    grid = (-10, -12, 40, 30, 2, 2)
    m2 = openfdcm.exhaustive_rotation_search(fm, tmpls, angles, k=2, radius=3, window=grid, pivot=None)
    assert [r.tmpl_idx for r in m2] == list(dev.exhaustive_rotation_search(tset, grid, cs, None, k=2, rx=3, ry=3)["tmpl_idx"])
    wide = np.array([[-400.0, 0.0, dev.width + 400.0, 0.0]], dtype=np.float32).T.copy()
    assert len(openfdcm.exhaustive_rotation_search(dev, [wide], angles, k=3, radius=2)) == 0


def test_bad_arguments_then_a_valid_call(built_pair, ragged):
    from openfdcm_amd import _capi as capi
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates, _rotations
    import ctypes as C
    scene, dev, orc = built_pair
    tmpls, tset = ragged
    good = (-60, -60, 50, 40, 2, 2)
    want = dev.exhaustive_rotation_search(tset, good, CS, None, k=3, rx=2, ry=2, ra=1, wrap=True)
    assert len(want) > 0
    bad_piv = np.zeros((len(tmpls), 2), dtype=np.float32)
    bad_piv[3, 1] = np.nan
    cases = [(CS, None, 0, 1, 1, 1, 1), (CS, None, 3, 33, 1, 1, 1), (CS, None, 3, 1, 1, 40, 0), (CS, None, 3, 1, 1, 1, 2),
             (np.float32([[1, np.inf]]), None, 3, 1, 1, 1, 1), (CS, bad_piv, 3, 1, 1, 1, 1)]
    for cs, pv, k, rx, ry, ra, wrap in cases:
        rot, keep = _rotations(cs, pv, tset.count)
        out, n = C.c_void_p(), C.c_int64()
        g = capi.Grid(*good)
        assert capi.lib().fdcm_search_exhaustive_rotations(dev._h, tset._h, C.byref(rot), C.byref(g), k, rx, ry, ra, wrap, 0,
                                                           C.byref(out), C.byref(n)) == -1
        if (k, rx, ra, wrap) == (3, 1, 1, 1):  # the rotation values themselves are bad: the score map refuses them too
            assert capi.lib().fdcm_score_map_rotations(dev._h, tset._h, C.byref(rot), C.byref(g),
                                                       capi.fptr(np.zeros(1, np.float32))) == -1
        assert dev.exhaustive_rotation_search(tset, good, CS, None, k=3, rx=2, ry=2, ra=1, wrap=True).tobytes() == want.tobytes()
    empty = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    assert len(empty.exhaustive_rotation_search(DeviceTemplates([tmpls[3]]), good, CS, k=3, rx=1, ry=1, ra=1)) == 0
    assert len(dev.exhaustive_rotation_search(DeviceTemplates([]), good, CS, k=3)) == 0
