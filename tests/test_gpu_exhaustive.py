"""GPU tests of the exhaustive translation search (include/fdcm.h, "exhaustive translation search"): the dense score map
and the top-k against the oracle's evaluate<Dt3Cpu> and against the seam (fdcm_featuremap_evaluate) bit for bit, the
admissible set and the default window against brute force, the public Python surface, config 2' at full size and the
64-bit addressing path of volumes above 4 GB."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

EINVAL = -1


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _grid_points(grid):
    """(ny, nx, 2) float32 translations of a grid (x0, y0, nx, ny, sx, sy)."""
    x0, y0, nx, ny, sx, sy = grid
    xs = (x0 + sx * np.arange(nx)).astype(np.float32)
    ys = (y0 + sy * np.arange(ny)).astype(np.float32)
    return np.stack(np.meshgrid(xs, ys), axis=-1)


def _seam_map(dev, tmpls, grid):
    """The seam at every grid point: (T, ny, nx) float32 from one fdcm_featuremap_evaluate call."""
    pts = _grid_points(grid).reshape(-1, 2)
    got = dev.evaluate(tmpls, [pts] * len(tmpls))
    return np.stack(got).reshape(len(tmpls), grid[3], grid[2])


def _host_topk(plane, k):
    """The first k admissible points of one template's map by (score, g): (g, score) arrays."""
    flat = plane.reshape(-1)
    g = np.flatnonzero(~np.isnan(flat))
    order = np.lexsort((g, flat[g]))
    g = g[order][:k]
    return g, flat[g]


def _check_topk(recs, maps, grid, k, base=0, skip=()):
    """recs: the raw records of one exhaustive search; maps: (T, ny, nx) score maps of the same grid."""
    x0, y0, nx, ny, sx, sy = grid
    pos = 0
    for t in range(maps.shape[0]):
        if t in skip:
            continue
        g, s = _host_topk(maps[t], k)
        r = recs[pos:pos + len(g)]
        pos += len(g)
        assert np.all(r["tmpl_idx"] == t + base), t
        assert _same_bits(r["score"], s), (t, r["score"][:5], s[:5])
        want = np.zeros((len(g), 6), dtype=np.float32)
        want[:, 0] = want[:, 4] = 1
        want[:, 2] = x0 + (g % nx) * sx
        want[:, 5] = y0 + (g // nx) * sy
        assert np.array_equal(r["transform"], want), t
    assert pos == len(recs)


def _templates_with_sizes(rng, S, sizes):
    out = []
    for n in sizes:
        c = rng.uniform(0.3 * S, 0.7 * S, size=2)
        pts = c[:, None] + rng.uniform(-0.2 * S, 0.2 * S, size=(2, 2 * n))
        out.append(pts.astype(np.float32).reshape(4, n, order="F"))
    return out


# n < 4, 4..7, >= 8 with and without tails (n % 4, n % 8), one empty template
SIZES = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 15, 16, 17, 20, 23, 24, 28, 31, 32, 36, 40]


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
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    rng = np.random.default_rng(23)
    tmpls = _templates_with_sizes(rng, dev.width / 1.2, SIZES)
    # one template that spans nearly the whole map: only a handful of admissible translations
    W = float(dev.width)
    tmpls.append(np.array([[-24.0, -24.0, W - 29.5, W - 28.0], [-20.0, W - 30.0, W - 28.7, -23.0]], dtype=np.float32).T.copy())
    return tmpls, DeviceTemplates(tmpls)


# windows partly outside every template's admissible box (the map is 307 x 307, scene translation 25.5: the random
# templates' boxes begin between x = -230 and -51 and end between 51 and 231)
GRIDS = [(-240, -60, 200, 120, 1, 1), (-241, -200, 160, 200, 3, 2)]


@pytest.mark.parametrize("grid", GRIDS)
def test_map_against_oracle_and_seam(built_pair, ragged, grid):
    """Every admissible point equals the oracle's evaluate<Dt3Cpu> bit for bit; the NaN pattern, and the whole map,
    equal the seam's at the same explicit translations."""
    scene, dev, orc = built_pair
    tmpls, tset = ragged
    got = dev.score_map(tset, grid)
    seam = _seam_map(dev, tmpls, grid)
    assert got.shape == (len(tmpls), grid[3], grid[2])
    assert np.array_equal(np.isnan(got), np.isnan(seam))
    assert _same_bits(got, seam)
    pts = _grid_points(grid).reshape(-1, 2)
    n_adm = 0
    for t, tm in enumerate(tmpls):
        flat = got[t].reshape(-1)
        adm = ~np.isnan(flat)
        if tm.shape[1] == 0:
            assert np.all(flat == 0) and not np.signbit(flat).any()
            continue
        assert not adm.all() and (adm.any() or t == len(tmpls) - 1), t  # the window crosses the admissible box
        want = O.evaluate(orc, tm, pts[adm])
        assert _same_bits(flat[adm], want), t
        n_adm += int(adm.sum())
    assert n_adm > 20000


def test_map_device_output(built_pair, ragged):
    """fdcm_score_map_device writes the same map into a caller's device buffer."""
    torch = pytest.importorskip("torch")
    scene, dev, orc = built_pair
    tmpls, tset = ragged
    grid = GRIDS[1]
    buf = torch.full((len(tmpls), grid[3], grid[2]), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dev.score_map_into(tset, grid, buf.data_ptr())
    assert _same_bits(buf.cpu().numpy(), dev.score_map(tset, grid))


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("k", [1, 5, 64])
def test_topk_against_the_map(built_pair, ragged, grid, k):
    """Per template with lines: its first k admissible points by (score, g), templates with fewer than k admissible points
    included; the empty template emits nothing."""
    scene, dev, orc = built_pair
    tmpls, tset = ragged
    maps = dev.score_map(tset, grid)
    recs = dev.exhaustive_search(tset, grid, k=k)
    counts = (~np.isnan(maps)).reshape(len(tmpls), -1).sum(axis=1)
    assert counts[-1] < 64  # the wide template has fewer points than the largest k
    _check_topk(recs, maps, grid, k, skip={0})


def test_topk_ties_are_grid_order():
    """An all-zero volume: every score is 0 and the order is pure grid order."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    dev = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 40, 30), dtype=np.float32), (0.0, 0.0))
    tmpls = [np.array([[2, 3, 10, 12], [5, 5, 6, 20]], dtype=np.float32).T.copy(),
             np.array([[1, 1, 2, 2]], dtype=np.float32).T.copy()]
    tset = DeviceTemplates(tmpls)
    grid = (-5, -4, 37, 29, 1, 1)
    maps = dev.score_map(tset, grid)
    assert np.all(maps[~np.isnan(maps)] == 0)
    for k in (1, 7, 64):
        recs = dev.exhaustive_search(tset, grid, k=k)
        assert np.all(recs["score"] == 0)
        _check_topk(recs, maps, grid, k)


def test_known_answer_shifted_scene_lines():
    """A template made of scene lines shifted by (-dx, -dy): top-1 scores 0, and (dx, dy) is among the score-0 records."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    S = 256
    segs = [(0, 0, S / 8, 0), (S - 1, S - 1, S - 1 - S / 8, S - 1), (40, 60, 120, 60), (40, 60, 40, 150), (200, 30, 200, 110),
            (90, 200, 180, 200), (150, 120, 230, 120), (70, 100, 70, 180)]
    scene = np.array(segs, dtype=np.float32).T.copy()
    dev = DeviceFeatureMap.build(scene, depth=12, coeff=5.0, padding=1.0, distance=0)
    assert tuple(dev.scene_translation) == (0.0, 0.0)
    dx, dy = 7, -5
    tmpl = (scene[:, 2:7] - np.array([dx, dy, dx, dy], dtype=np.float32)[:, None]).astype(np.float32)
    tset = DeviceTemplates([tmpl])
    grid = (dx - 6, dy - 6, 13, 13, 1, 1)
    recs = dev.exhaustive_search(tset, grid, k=5)
    assert recs[0]["score"] == 0
    zero = recs[recs["score"] == 0]
    assert any(r["transform"][2] == dx and r["transform"][5] == dy for r in zero)
    # the default window holds it too
    import openfdcm_amd as openfdcm
    best = openfdcm.exhaustive_search(dev, [tmpl], k=1)
    assert best[0].score == 0


def _brute_box(dev, tm, box):
    """Admissible integer translations of one template inside box = (x0, y0, x1, y1), through the seam."""
    x0, y0, x1, y1 = box
    grid = (x0, y0, x1 - x0 + 1, y1 - y0 + 1, 1, 1)
    m = _seam_map(dev, [tm], grid)[0]
    jj, ii = np.nonzero(~np.isnan(m))
    return ii + x0, jj + y0


@pytest.mark.parametrize("stride", [(1, 1), (3, 2), (5, 7)])
def test_default_window_against_brute_force(built_pair, stride):
    scene, dev, orc = built_pair
    from openfdcm_amd.engine import DeviceTemplates
    rng = np.random.default_rng(31)
    tmpls = _templates_with_sizes(rng, dev.width / 1.2, [3, 9, 17])
    tmpls.append(np.zeros((4, 0), dtype=np.float32))  # no lines: does not widen the window
    W = dev.width
    box = (-W, -W, W, W)
    xs, ys = [], []
    for tm in tmpls[:3]:
        x, y = _brute_box(dev, tm, box)
        assert len(x) and x.min() > -W and x.max() < W and y.min() > -W and y.max() < W
        xs.append(x); ys.append(y)
    xs, ys = np.concatenate(xs), np.concatenate(ys)
    sx, sy = stride
    g = dev.exhaustive_window(DeviceTemplates(tmpls), sx, sy).as_tuple()
    x0, y0 = (xs.min() // sx) * sx, (ys.min() // sy) * sy
    assert g == (x0, y0, (xs.max() - x0) // sx + 1, (ys.max() - y0) // sy + 1, sx, sy)
    # nothing fits: a template wider than the map, or only templates without lines
    wide = np.array([[-40.0, 0.0, W + 40.0, 0.0]], dtype=np.float32).T.copy()
    assert dev.exhaustive_window(DeviceTemplates([wide]), sx, sy).as_tuple()[2:4] == (0, 0)
    assert dev.exhaustive_window(DeviceTemplates([np.zeros((4, 0), dtype=np.float32)]), sx, sy).as_tuple()[2:4] == (0, 0)
    import openfdcm_amd as openfdcm
    assert len(openfdcm.exhaustive_search(dev, [wide], stride=stride, k=3)) == 0
    m, gg = openfdcm.score_map(dev, [wide], stride=stride)
    assert m.shape == (1, 0, 0) and gg[2:4] == (0, 0)


def test_empty_inputs_give_zero_records(built_pair):
    """A feature map of size 0, or an empty template list: zero records, no error."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    scene, dev, orc = built_pair
    empty = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    tm = [np.array([[1, 1, 2, 2]], dtype=np.float32).T.copy(), np.zeros((4, 0), dtype=np.float32)]
    tset = DeviceTemplates(tm)
    grid = (0, 0, 5, 4, 1, 1)
    assert len(empty.exhaustive_search(tset, grid, k=3)) == 0
    m = empty.score_map(tset, grid)
    assert np.isnan(m[0]).all() and np.all(m[1] == 0)
    assert empty.exhaustive_window(tset, 1, 1).as_tuple()[2:4] == (0, 0)
    none = DeviceTemplates([])
    assert len(dev.exhaustive_search(none, grid, k=3)) == 0
    assert dev.score_map(none, grid).shape == (0, 4, 5)


def test_public_api(built_pair):
    import openfdcm_amd as openfdcm
    from openfdcm_amd.engine import DeviceTemplates
    scene, dev, orc = built_pair
    rng = np.random.default_rng(41)
    tmpls = _templates_with_sizes(rng, dev.width / 1.2, [6, 12, 0, 20])
    fm = openfdcm.build_cpu_featuremap(scene, openfdcm.Dt3CpuParameters(depth=12, dt3Coeff=5.0, padding=1.2))
    matches = openfdcm.exhaustive_search(fm, tmpls, stride=(4, 3), k=3)
    assert len(matches) == 9 and sorted({m.tmpl_idx for m in matches}) == [0, 1, 3]
    for m in matches:
        tr = np.asarray(m.transform)
        assert tr.shape == (2, 3) and np.array_equal(tr[:, :2], np.eye(2))
    lengths = openfdcm.get_template_lengths(tmpls)
    ranked = openfdcm.sort_matches(openfdcm.penalize(openfdcm.ExponentialPenalty(1.5), matches, lengths))
    assert len(ranked) == 9 and all(ranked[i].score <= ranked[i + 1].score for i in range(8))
    win = openfdcm.exhaustive_window(fm, tmpls, stride=(4, 3))
    maps, g = openfdcm.score_map(openfdcm.FeatureMap(fm), tmpls, stride=(4, 3))
    assert g == win and maps.shape == (4, g[3], g[2])
    _check_topk(matches.records(), maps, g, 3, skip={2})
    # an explicit window, and tmpl_index_base
    grid = (-10, -12, 40, 30, 2, 2)
    m2 = openfdcm.exhaustive_search(fm, tmpls, k=2, window=grid)
    raw = dev.exhaustive_search(DeviceTemplates(tmpls), grid, k=2, tmpl_index_base=100)
    assert [m.tmpl_idx for m in m2] == [t - 100 for t in raw["tmpl_idx"]]
    assert np.all(raw["tmpl_idx"] >= 100)


def test_config2p_full_size():
    """Config 2' (1024^2, depth 30, 1000 templates x 32 lines), stride 4, k = 4: every record is the oracle's score at
    its translation, and 50 templates' top-k equal the host's top-k of their score map."""
    from openfdcm_amd import synthetic
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    cfg, scene, tmpls = synthetic.make_config("2p")
    dev = DeviceFeatureMap.build(scene, depth=cfg["depth"], coeff=5.0, padding=1.0, distance=cfg["distance"])
    orc = O.build(scene, depth=cfg["depth"], coeff=5.0, padding=1.0, distance=cfg["distance"], nthreads=16)
    tset = DeviceTemplates(tmpls)
    grid = dev.exhaustive_window(tset, 4, 4).as_tuple()
    assert grid[2] > 200 and grid[3] > 200
    recs = dev.exhaustive_search(tset, grid, k=4)
    assert len(recs) == 4 * len(tmpls)
    for t in range(len(tmpls)):
        r = recs[4 * t:4 * t + 4]
        assert np.all(r["tmpl_idx"] == t)
        want = O.evaluate(orc, tmpls[t], r["transform"][:, [2, 5]])
        assert _same_bits(r["score"], want), t
    sub = list(range(0, 1000, 20))
    maps = dev.score_map(DeviceTemplates([tmpls[t] for t in sub]), grid)
    for q, t in enumerate(sub):
        g, s = _host_topk(maps[q], 4)
        assert _same_bits(recs[4 * t:4 * t + 4]["score"], s), t
        assert np.array_equal(recs[4 * t:4 * t + 4]["transform"][:, 2], grid[0] + (g % grid[2]) * grid[4])
        assert np.array_equal(recs[4 * t:4 * t + 4]["transform"][:, 5], grid[1] + (g // grid[2]) * grid[5])


def test_volume_above_4gb_uses_64bit_addresses():
    """Config 5's feature map (4096^2, depth 180, L1: 12 GB): 16 templates at stride 64, the map equals the seam."""
    from openfdcm_amd import synthetic
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    cfg = synthetic.CONFIGS["5"]
    scene = synthetic.scene(cfg["S"], cfg["scene_lines"], 1)
    tmpls = synthetic.templates(16, cfg["n"], cfg["S"], 2)
    dev = DeviceFeatureMap.build(scene, depth=cfg["depth"], coeff=5.0, padding=1.0, distance=cfg["distance"])
    assert dev.depth * dev.device_slice_stride() * 4 >= 1 << 32
    tset = DeviceTemplates(tmpls)
    grid = dev.exhaustive_window(tset, 64, 64).as_tuple()
    grid = (grid[0] - 128, grid[1] - 64, grid[2] + 4, grid[3] + 3, 64, 64)  # past the admissible box on every side
    got = dev.score_map(tset, grid)
    seam = _seam_map(dev, tmpls, grid)
    assert _same_bits(got, seam)
    assert np.isnan(got).any() and (~np.isnan(got)).sum() > 16 * 1000
    recs = dev.exhaustive_search(tset, grid, k=8)
    _check_topk(recs, got, grid, 8)
    dev.close()


def test_bad_arguments_then_a_valid_call(built_pair, ragged):
    from openfdcm_amd import _capi as capi
    scene, dev, orc = built_pair
    tmpls, tset = ragged
    lib = capi.lib()
    good = capi.Grid(-20, -20, 30, 30, 2, 2)
    want = dev.exhaustive_search(tset, good, k=3)
    bad = [(capi.Grid(-20, -20, 30, 30, 0, 2), 3), (capi.Grid(-20, -20, 30, 30, 2, 2), 0),
           (capi.Grid(-20, -20, 30, 30, 2, 2), 65), (capi.Grid(0, 0, 1 << 16, 1 << 15, 1, 1), 3)]
    for g, k in bad:
        out, n = C.c_void_p(), C.c_int64()
        assert lib.fdcm_search_exhaustive(dev._h, tset._h, C.byref(g), k, 0, C.byref(out), C.byref(n)) == EINVAL
        assert lib.fdcm_last_error()
        got = dev.exhaustive_search(tset, good, k=3)
        assert got.tobytes() == want.tobytes()
    out = np.zeros(4, dtype=np.float32)
    assert lib.fdcm_score_map(dev._h, tset._h, C.byref(capi.Grid(0, 0, 2, 2, 0, 1)), capi.fptr(out)) == EINVAL
    assert lib.fdcm_exhaustive_window(dev._h, tset._h, 0, 1, C.byref(capi.Grid())) == EINVAL
    assert _same_bits(dev.score_map(tset, good), _seam_map(dev, tmpls, good.as_tuple()))
    # translations past |t| < 2^24 are outside the stated range
    far = capi.Grid((1 << 24) - 10, 0, 20, 2, 1, 1)
    o2, n2 = C.c_void_p(), C.c_int64()
    assert lib.fdcm_search_exhaustive(dev._h, tset._h, C.byref(far), 1, 0, C.byref(o2), C.byref(n2)) == EINVAL
    assert "2^24" in lib.fdcm_last_error().decode()
