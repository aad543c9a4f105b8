"""Every scorer on adopted non-square volumes, on built maps of every distance and on volumes with non-finite data, against
definitions that come from neither restatement of the reference.

The volume is interleaved on the device (pixel (k, x, y) at k SL + ((x >> 2) H + y) 4 + (x & 3)), so an addressing
mistake that swaps W and H, or a wrong slice stride when W % 4 != 0, reads a wrong pixel of a non-square map and nothing
at all of a square one.  Here the maps are adopted at widths and heights from 1 to 1030 in both orders, with three kinds
of content:

  pixel   v(k, x, y) = k W H + x H + y: every pixel a different integer below 2^24, so a wrong read changes the score
  int     small non-negative integers: every partial sum is exact, the score is the integer sum bit for bit
  float   random float32 over seven decades

The definitions, in numpy:

  admissible   t is admissible for a template when fl(p + fl(T + t)) lies in (-1, W) (x) or (-1, H) (y) for every end
               point coordinate p, T the scene translation, every operation float32 (the seam's rule)
  score        the template's terms |v(bin, trunc q1) - v(bin, trunc q2)| in float32, bin the float64-nearest key, added
               in Eigen 3.4's redux order (fdcm_score.h): exact bits on every kind; also held to the float64 rescore
  keys         (score bits << 32) | index for an admissible point whose score is not NaN (tests/peaks_ref.py,
               tests/rotation_ref.py applied to the definition maps, not to the device's)

Each check runs on the oracle (CPU) and on the device (`gpu`) from one parametrisation where the oracle offers the
operation (evaluate, search, minmaxTranslation); the exhaustive search is the device's alone.
"""
import numpy as np
import pytest

from helpers import EDGE_SCENES, FMAX, definition_keys, f32, nearest_bins, rescore, ulp32
from oracle import oracle as O
from peaks_ref import peaks_ref
from rotation_ref import rotate_lines, rotation_peaks_ref

BACKENDS = [pytest.param("oracle", id="oracle"), pytest.param("device", id="device", marks=pytest.mark.gpu)]
DISTS = [pytest.param(O.L2, id="l2"), pytest.param(O.L2_SQUARED, id="l2sq"), pytest.param(O.L1, id="l1")]

# name: (W, H, depth, scene translation).  W % 4 takes every value; some maps sit far from the origin.
ADOPTED = {"1x1": (1, 1, 1, (0.0, 0.0)), "1x37": (1, 37, 3, (0.5, -3.25)), "37x1": (37, 1, 12, (0.0, 0.0)),
           "3x700": (3, 700, 1, (5000.3, -12345.7)), "700x3": (700, 3, 12, (-0.375, 0.0)), "5x64": (5, 64, 12, (-2.75, 0.125)),
           "64x5": (64, 5, 180, (0.0, 0.0)), "257x31": (257, 31, 3, (5000.3, -12345.7)), "31x257": (31, 257, 12, (0.0, 0.0)),
           "1030x17": (1030, 17, 1, (-40.5, 7.0)), "17x1030": (17, 1030, 180, (0.0, 3.5))}
KINDS = ["pixel", "int", "float"]
SIZES = [1, 1, 1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 17]   # lines per template: n < 4, 4..7, >= 8 with and without tails


# ------------------------------------------------------------------------------------------------ definitions
def make_volume(kind, m, W, H, seed):
    rng = np.random.default_rng(seed)
    if kind == "pixel":
        return np.arange(m * W * H, dtype=np.float64).reshape(m, W, H).astype(np.float32)
    if kind == "int":
        return rng.integers(0, 16, size=(m, W, H)).astype(np.float32)
    vol = (rng.uniform(0, 1, size=(m, W, H)) * 10.0 ** rng.uniform(-3, 4, size=(m, W, H))).astype(np.float32)
    if kind == "nonfinite":   # scattered NaN, +inf, -inf and FLT_MAX pixels
        r = rng.uniform(size=vol.shape)
        vol[r < 0.15] = np.nan
        vol[(r >= 0.15) & (r < 0.18)] = np.inf
        vol[(r >= 0.18) & (r < 0.21)] = -np.inf
        vol[(r >= 0.21) & (r < 0.24)] = FMAX
    return vol


def eigen_sum32(terms):
    """(P, n) float32 -> (P,) float32: Eigen 3.4.0's redux order (Packet4f): p0 = packet 0, p1 = packet 1, blocks of 8
    p0 += packet(i), p1 += packet(i + 4); p0 += p1; the trailing packet; (p0[0] + p0[2]) + (p0[1] + p0[3]); the scalar
    tail in order.  Fewer than 4 terms: left to right."""
    with np.errstate(over="ignore", invalid="ignore"):
        return _eigen_sum32(np.asarray(terms, dtype=np.float32))


def _eigen_sum32(terms):
    P, n = terms.shape
    if n == 0:
        return np.zeros(P, dtype=np.float32)
    a2, a = (n // 8) * 8, (n // 4) * 4
    if a == 0:
        res = terms[:, 0].copy()
        for i in range(1, n):
            res = res + terms[:, i]
        return res
    p0 = terms[:, 0:4].copy()
    if a2 >= 8:
        p1 = terms[:, 4:8].copy()
        for b in range(8, a2, 8):
            p0 = p0 + terms[:, b:b + 4]
            p1 = p1 + terms[:, b + 4:b + 8]
        p0 = p0 + p1
        if a > a2:
            p0 = p0 + terms[:, a2:a2 + 4]
    res = (p0[:, 0] + p0[:, 2]) + (p0[:, 1] + p0[:, 3])
    for i in range(a, n):
        res = res + terms[:, i]
    return res


def bins_of(lines, m):
    b, amb = nearest_bins(np.asarray(lines, dtype=np.float64), m, 1e-5)
    assert not amb.any(), "a template line lies on a bin boundary: choose another seed"
    return b


def axis_admissible(p_lo, p_hi, Toff, ts, size):
    """(len(ts),) bool: fl(p + fl(T + t)) in (-1, size) for the extreme end point coordinates p_lo, p_hi, in float32."""
    off = f32(Toff) + np.asarray(ts, dtype=np.int64).astype(np.float32)
    return (f32(p_lo) + off > f32(-1)) & (f32(p_hi) + off < f32(size))


def definition_map(vol, tmpl, T, grid):
    """(ny, nx) float32: the score of the (4, n) template at every point of the grid, NaN where not admissible."""
    x0, y0, nx, ny, sx, sy = grid
    m, W, H = vol.shape
    tmpl = np.asarray(tmpl, dtype=np.float32)
    b = bins_of(tmpl, m)
    offx = f32(T[0]) + (x0 + sx * np.arange(nx, dtype=np.int64)).astype(np.float32)
    offy = f32(T[1]) + (y0 + sy * np.arange(ny, dtype=np.int64)).astype(np.float32)
    qx = tmpl[[0, 2]][None, :, :] + offx[:, None, None]           # (nx, 2, n) float32
    qy = tmpl[[1, 3]][None, :, :] + offy[:, None, None]
    okx = ((qx > -1) & (qx < W)).all(axis=(1, 2))
    oky = ((qy > -1) & (qy < H)).all(axis=(1, 2))
    out = np.full((ny, nx), np.nan, dtype=np.float32)
    ii, jj = np.flatnonzero(okx), np.flatnonzero(oky)
    if len(ii) == 0 or len(jj) == 0:
        return out
    ix = np.trunc(qx[ii]).astype(np.int64)                         # (ni, 2, n)
    iy = np.trunc(qy[jj]).astype(np.int64)                         # (nj, 2, n)
    a = vol[b[None, None, :], ix[None, :, 0, :], iy[:, None, 0, :]]   # (nj, ni, n)
    c = vol[b[None, None, :], ix[None, :, 1, :], iy[:, None, 1, :]]
    with np.errstate(invalid="ignore"):
        terms = np.abs(a - c)
    s = eigen_sum32(terms.reshape(-1, tmpl.shape[1])).reshape(len(jj), len(ii))
    out[np.ix_(jj, ii)] = s
    return out


def admissible_box(tmpl, T, W, H):
    """The integer translations whose every end point is admissible: (x0, x1, y0, y1) by brute force over a range that
    holds the whole set, or None."""
    tmpl = np.asarray(tmpl, dtype=np.float32)
    out = []
    for lo, hi, Toff, size in ((tmpl[[0, 2]].min(), tmpl[[0, 2]].max(), T[0], W),
                               (tmpl[[1, 3]].min(), tmpl[[1, 3]].max(), T[1], H)):
        a = int(np.floor(-1.0 - float(hi) - float(Toff))) - 3
        b = int(np.ceil(float(size) - float(lo) - float(Toff))) + 3
        ts = np.arange(a, b + 1)
        ok = axis_admissible(lo, hi, Toff, ts, size)
        assert not ok[0] and not ok[-1]
        if not ok.any():
            return None
        idx = np.flatnonzero(ok)
        assert idx[-1] - idx[0] + 1 == len(idx)                         # an interval
        out += [int(ts[idx[0]]), int(ts[idx[-1]])]
    return tuple(out)


def random_templates(rng, W, H, T, m, sizes, span=0.6, margin=1e-4):
    """Templates in scene coordinates whose end points fall in the map at translation 0 (roughly), extent up to `span`
    of the map, no line on a bin boundary."""
    out = []
    for n in sizes:
        while True:
            c = rng.uniform(0, 1, size=2) * (W, H)
            e = (rng.uniform(-0.5, 0.5, size=(2, 2 * n)) * span * np.array([[max(W - 1, 0.9)], [max(H - 1, 0.9)]]))
            pts = c[:, None] + e - np.asarray(T, dtype=np.float64)[:, None]
            t = pts.astype(np.float32).reshape(4, n, order="F")
            if (np.hypot(t[2] - t[0], t[3] - t[1]) > 1e-3).all() and not nearest_bins(t.astype(np.float64), m, margin)[1].any():
                out.append(t)
                break
    return out


def boundary_template(W, H, T, axis, m):
    """One line whose far end point sits where float32 and exact arithmetic disagree on admissibility: for some integer t,
    fl(p + fl(T + t)) == size while p + fl(T + t) < size.  None when the map is too small for such a point."""
    size, Toff = (W, T[0]) if axis == 0 else (H, T[1])
    if size < 256:
        return None
    t = int(np.floor(size - 1.5 - float(Toff)))
    off = f32(Toff) + f32(t)
    p = f32(float(size) - float(off))
    for _ in range(200):   # the largest float32 p with p + off < size exactly
        if float(p) + float(off) < size:
            break
        p = np.nextafter(p, f32(-np.inf))
    if not (f32(p) + off >= f32(size)):
        return None
    other = f32(p - f32(0.75 * size))
    across = H if axis == 0 else W
    q = f32(0.3 * across) - f32(T[1] if axis == 0 else T[0])
    for d in (0.4, 0.25, 0.1, 0.55):   # a direction off every bin boundary
        e = f32(d * across)
        t = np.array([other, q, p, q + e] if axis == 0 else [q, other, q + e, p], dtype=np.float32).reshape(4, 1)
        if not nearest_bins(t.astype(np.float64), m, 1e-4)[1].any():
            return t
    return None


def adopted(name, kind, seed=0):
    W, H, m, T = ADOPTED[name]
    return make_volume(kind, m, W, H, seed + 7 * m + W), definition_keys(m).astype(np.float32), np.array(T, dtype=np.float32)


def adopted_templates(name, seed):
    W, H, m, T = ADOPTED[name]
    rng = np.random.default_rng(seed + W * 31 + H)
    tm = random_templates(rng, W, H, T, m, SIZES)
    for axis in (0, 1):
        b = boundary_template(W, H, T, axis, m)
        if b is not None:
            tm.append(b)
    return tm


def device_map(vol, keys, T, via):
    """The adopted volume on the device: a DeviceFeatureMap.from_volume, or an openfdcm.FeatureMap of openfdcm.Dt3Cpu's
    {key: (H, W)} dict (the reference's constructor and its Python transpose).  Both offer evaluate and
    minmax_translation, and every openfdcm exhaustive-search function takes either."""
    if via == "volume":
        from openfdcm_amd.engine import DeviceFeatureMap
        return DeviceFeatureMap.from_volume(keys, vol, T)
    import openfdcm_amd as openfdcm
    m, W, H = vol.shape
    return openfdcm.FeatureMap(openfdcm.Dt3Cpu({float(k): np.ascontiguousarray(vol[i].T) for i, k in enumerate(keys)}, T,
                                               (W, H)))


def _assert_same_bits(got, want, what):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    if bad.any():
        idx = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; first at {idx}: got {got[idx]!r} "
                             f"definition {want[idx]!r}")


def _same_records(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    assert np.array_equal(got["tmpl_idx"], want["tmpl_idx"]), what
    _assert_same_bits(got["score"], want["score"], what + " score")
    _assert_same_bits(got["transform"], want["transform"], what + " transform")


def _grid_points(grid):
    x0, y0, nx, ny, sx, sy = grid
    xs = (x0 + sx * np.arange(nx)).astype(np.float32)
    ys = (y0 + sy * np.arange(ny)).astype(np.float32)
    return np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)


def _covering_grid(boxes, stride, margin):
    """A grid with the given stride that runs past the union of the boxes by `margin` points on every side."""
    sx, sy = stride
    bx = [b for b in boxes if b is not None]
    x_lo, x_hi = min(b[0] for b in bx), max(b[1] for b in bx)
    y_lo, y_hi = min(b[2] for b in bx), max(b[3] for b in bx)
    x0, y0 = x_lo - margin * sx - 1, y_lo - margin * sy - 2
    return (x0, y0, (x_hi - x0) // sx + margin + 1, (y_hi - y0) // sy + margin + 1, sx, sy)


def _window_definition(boxes, stride):
    sx, sy = stride
    bx = [b for b in boxes if b is not None]
    if not bx:
        return None
    x_lo, x_hi = min(b[0] for b in bx), max(b[1] for b in bx)
    y_lo, y_hi = min(b[2] for b in bx), max(b[3] for b in bx)
    x0, y0 = (x_lo // sx) * sx, (y_lo // sy) * sy
    return (x0, y0, (x_hi - x0) // sx + 1, (y_hi - y0) // sy + 1, sx, sy)


# ------------------------------------------------------------------------------------------------ 0. the definitions
def test_eigen_sum32_is_the_redux_order():
    """eigen_sum32 against the oracle's restatement of Eigen's sum at every length up to 40 (the order, not the value:
    random magnitudes over seven decades make every order give other bits)."""
    rng = np.random.default_rng(5)
    for n in range(41):
        v = (rng.uniform(0, 1, size=(64, n)) * 10.0 ** rng.uniform(-3, 4, size=(64, n))).astype(np.float32)
        want = np.array([O.eigen_sum(np.ascontiguousarray(r)) for r in v], dtype=np.float32)
        assert np.array_equal(eigen_sum32(v).view(np.uint32), want.view(np.uint32)), n


def test_boundary_templates_exist():
    """The wide maps get a template whose admissible box float32 and exact arithmetic disagree on."""
    got = [n for n in ADOPTED if any(boundary_template(*ADOPTED[n][:2], ADOPTED[n][3], a, ADOPTED[n][2]) is not None
                                     for a in (0, 1))]
    assert {"1030x17", "17x1030", "700x3", "3x700", "257x31", "31x257"} <= set(got), got


# ------------------------------------------------------------------------------------------------ A. adopted volumes
def _evaluate(backend, fm, tmpl, trs):
    if backend == "oracle":
        return O.evaluate(fm, tmpl, trs)
    return fm.evaluate([tmpl], [trs])[0]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(ADOPTED))
def test_adopted_evaluate_is_the_definition(backend, kind, name):
    """evaluate at random translations around every template's admissible box: NaN exactly where the float32 rule puts an
    end point outside (-1, W) x (-1, H) (device; the oracle reads unchecked and is given admissible points only), the
    definition's bits at admissible points, within the float64 rescore's bound, and (device) O.evaluate's bits."""
    vol, keys, T = adopted(name, kind)
    m, W, H = vol.shape
    orc = O.from_volume(keys, vol, T)
    fm = orc if backend == "oracle" else device_map(vol, keys, T, "volume")
    rng = np.random.default_rng(len(name) + m)
    n_adm = n_out = 0
    for tm in adopted_templates(name, 1):
        box = admissible_box(tm, T, W, H)
        if box is None:
            continue
        g = (box[0] - 3, box[2] - 3, box[1] - box[0] + 7, box[3] - box[2] + 7, 1, 1)
        pts = _grid_points(g)
        pts = pts[rng.choice(len(pts), size=min(len(pts), 300), replace=False)]
        dmap = definition_map(vol, tm, T, g)
        want = dmap[(pts[:, 1] - g[1]).astype(int), (pts[:, 0] - g[0]).astype(int)]
        adm = ~np.isnan(want)
        ix = pts.astype(np.int64)
        in_box = (ix[:, 0] >= box[0]) & (ix[:, 0] <= box[1]) & (ix[:, 1] >= box[2]) & (ix[:, 1] <= box[3])
        assert np.array_equal(adm, in_box), name
        use = adm if backend == "oracle" else np.ones(len(pts), dtype=bool)
        got = _evaluate(backend, fm, tm, pts[use])
        _assert_same_bits(got, want[use], f"{backend} {name} {kind}")
        if backend == "device":
            _assert_same_bits(got[adm], O.evaluate(orc, tm, pts[adm]), f"seam vs oracle {name} {kind}")
        # float64: the score is the sum of the terms within n 2^-24 sum|terms|
        for p, s in zip(pts[adm][:20], want[adm][:20]):
            lines = tm.astype(np.float64) + (np.array([T[0] + p[0], T[1] + p[1]] * 2, dtype=np.float32)
                                             .astype(np.float64)[:, None])
            r, bound, status = rescore(vol, keys, lines, W, H, max(1e-3, 2 * ulp32(lines)), ulp32(tm))
            if status == "ok":
                assert abs(float(s) - r) <= bound, (name, float(s), r)
        n_adm += int(adm.sum())
        n_out += int((~adm).sum())
    assert n_adm > 10 and n_out > 10, (n_adm, n_out)


def minmax_definition(tmpl, av, W, H, T):
    """The multiplier interval of minmaxTranslation from its meaning: the (float32) bounding box p + T of the template
    moved by mu * av stays inside [0, W - 1] x [0, H - 1].  Per axis r with av_r != 0 that is the float64 interval
    -min_r / av_r .. (size_r - 1 - max_r) / av_r (ends swapped for av_r < 0), intersected over such axes.  (inf, inf) for
    a zero align vector, (NaN, NaN) when the box does not start inside the map."""
    tmpl = np.asarray(tmpl, dtype=np.float32)
    if av[0] == 0 and av[1] == 0:
        return np.inf, np.inf
    lo, hi = -np.inf, np.inf
    for r, size in ((0, W), (1, H)):
        mn = float(tmpl[[r, r + 2]].min() + f32(T[r]))
        mx = float(tmpl[[r, r + 2]].max() + f32(T[r]))
        if mn < 0 or size - 1 - mx < 0:
            return np.nan, np.nan
        if av[r] != 0:
            a, b = -mn / float(av[r]), (size - 1 - mx) / float(av[r])
            lo, hi = max(lo, min(a, b)), min(hi, max(a, b))
    return lo, hi


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(ADOPTED))
def test_adopted_minmax_translation(backend, name):
    """minmaxTranslation on every size against its definition within a few float32 roundings (the bounding box, one
    subtraction and one division), NaN and inf exactly; (device) bit for bit the oracle's, through from_volume (batched
    and single) and through Dt3Cpu."""
    vol, keys, T = adopted(name, "int")
    W, H = vol.shape[1:]
    rng = np.random.default_rng(W * 7 + H)
    tms, avs = [], []
    # and one template that fits a map one pixel wide or high: its box is [0, (W - 1) / 2] x [0, (H - 1) / 2] exactly
    fit = np.array([-T[0], -T[1], -T[0] + f32(0.5 * (W - 1)), -T[1] + f32(0.5 * (H - 1))], dtype=np.float32).reshape(4, 1)
    for tm in adopted_templates(name, 2) + [fit]:
        for av in ([1.0, 0.0], [0.0, 1.0], [0.6, -0.8], [-0.3, 0.1], [0.0, 0.0], rng.uniform(-1, 1, size=2)):
            tms.append(tm)
            avs.append(np.array(av, dtype=np.float32))
    want = np.stack([O.minmax_translation(t, a, (W, H), T) for t, a in zip(tms, avs)])
    inside = 0
    for (lo, hi), t, a in zip(want, tms, avs):
        dlo, dhi = minmax_definition(t, a, W, H, T)
        for g, d in ((lo, dlo), (hi, dhi)):
            if not np.isfinite(d):
                assert (np.isnan(g) and np.isnan(d)) or g == d, (name, t, a, g, d)
            else:
                # |p| + |T| + W bounds every value on the way: 4 ulps of it, divided by |av_r| >= min |av|
                scale = (np.abs(t).max() + np.abs(T).max() + max(W, H)) / np.abs(a[a != 0]).min()
                assert abs(float(g) - d) <= 4 * float(np.spacing(f32(scale))), (name, t, a, g, d)
                inside += 1
    assert inside >= 4, inside
    if backend == "device":
        dev = device_map(vol, keys, T, "volume")
        _assert_same_bits(dev.minmax_translation_batch(tms, np.stack(avs)), want, name)
        _assert_same_bits(np.stack([dev.minmax_translation(t, a) for t, a in zip(tms[:8], avs[:8])]), want[:8], name)
        fm = device_map(vol, keys, T, "dt3cpu")
        _assert_same_bits(np.stack([fm.minmax_translation(t, a) for t, a in zip(tms, avs)]), want, name + " Dt3Cpu")


def _scene_inside(rng, W, H, T, n):
    """Scene lines with both end points inside the map at translation 0."""
    p = rng.uniform(0, 1, size=(2, 2 * n)) * np.array([[W - 1], [H - 1]]) - np.asarray(T, dtype=np.float64)[:, None]
    s = p.astype(np.float32).reshape(4, n, order="F")
    s[2:] += (np.hypot(s[2] - s[0], s[3] - s[1]) < 1e-3) * f32(0.5)
    return s


SEARCH_MAPS = ["5x64", "64x5", "257x31", "31x257", "1030x17", "17x1030", "3x700", "700x3", "37x1", "1x37"]
OPTIMIZERS = [pytest.param((O.BATCH_OPTIMIZE, 10), id="batch"), pytest.param((O.DEFAULT_OPTIMIZE, 1), id="default"),
              pytest.param((O.INDULGENT_OPTIMIZE, 3), id="indulgent")]


def _search_records(backend, vol, keys, T, via, tmpls, scene, opt):
    kind, batch = opt
    if backend == "oracle":
        return O.search(O.from_volume(keys, vol, T), tmpls, scene, 4, 4, kind=kind, batch=batch, nthreads=4)
    import openfdcm_amd as openfdcm
    from openfdcm_amd.engine import DeviceTemplates, search_raw
    if via == "volume":
        return search_raw(device_map(vol, keys, T, via), DeviceTemplates(tmpls), scene, 4, 4, kind, batch)
    m, W, H = vol.shape
    dt3 = openfdcm.Dt3Cpu({float(k): np.ascontiguousarray(vol[i].T) for i, k in enumerate(keys)}, T, (W, H))
    optimizer = {O.BATCH_OPTIMIZE: openfdcm.BatchOptimize(batch), O.DEFAULT_OPTIMIZE: openfdcm.DefaultOptimize(),
                 O.INDULGENT_OPTIMIZE: openfdcm.IndulgentOptimize(batch)}[kind]
    res = openfdcm.search(openfdcm.DefaultMatch(), openfdcm.DefaultSearch(4, 4), optimizer, dt3, tmpls, scene)
    return openfdcm.records_of(res)


def _check_records_rescore(rec, vol, keys, T, tmpls, what):
    m, W, H = vol.shape
    st = T.astype(np.float64)
    skipped = 0
    for r in rec:
        Tm = r["transform"].astype(np.float64).reshape(2, 3)
        t = tmpls[r["tmpl_idx"]].astype(np.float64)
        pts = t.reshape(2, -1, order="F")
        moved = (Tm[:, :2] @ pts + Tm[:, 2:3] + st[:, None]).reshape(4, -1, order="F")
        big = max(ulp32(moved), ulp32(Tm[:, 2]), ulp32(st), ulp32(Tm[:, :2] @ pts))
        aligned = max(ulp32(Tm[:, :2] @ pts + Tm[:, 2:3]), ulp32(Tm[:, :2] @ pts))
        s, bound, status = rescore(vol, keys, moved, W, H, max(1e-3, 4 * big), 2 * aligned)
        if status != "ok":
            skipped += 1
            continue
        assert abs(float(r["score"]) - s) <= bound, (what, int(r["tmpl_idx"]), float(r["score"]), s, bound)
    # far from the origin float32 reaches 2^-10 of a pixel, and in a map a few pixels thin the walk stops where an end
    # point meets the map's edge: there more end points lie within reach of a pixel edge
    loose = np.abs(st).max() >= 1000 or min(W, H) < 8
    assert skipped <= (0.5 if loose else 0.25) * len(rec) + 2, (what, skipped, len(rec))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("opt", OPTIMIZERS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", SEARCH_MAPS)
def test_adopted_search_matches_oracle_and_rescores(backend, opt, kind, name):
    """DefaultSearch with every optimiser on an adopted volume, scene lines inside the map: (device) positionally
    bit-identical to O.search, through from_volume and through Dt3Cpu; every record re-scored from its own transform."""
    vol, keys, T = adopted(name, kind)
    m, W, H = vol.shape
    rng = np.random.default_rng(W + 3 * H + m)
    scene = _scene_inside(rng, W, H, T, 12)
    tmpls = random_templates(rng, W, H, T, m, [2, 3, 4, 5, 6, 8, 9], span=0.5)
    want = _search_records("oracle", vol, keys, T, None, tmpls, scene, opt)
    if backend == "device":
        for via in ("volume", "dt3cpu"):
            _same_records(_search_records("device", vol, keys, T, via, tmpls, scene, opt), want, f"{name} {kind} {via}")
    assert len(want) > 0 or min(W, H) < 5
    _check_records_rescore(want, vol, keys, T, tmpls, f"{name} {kind}")


# ---- the exhaustive search on adopted volumes (device only)
def _exhaustive_checks(fm, vol, keys, T, tmpls, grid, ks=(1, 8, 64), radii=((0, 0), (1, 0), (2, 5), (32, 32))):
    """score_map against the definition (bits) and the seam (bits), top-k and peaks against peaks_ref of the definition
    maps.  Returns the definition maps."""
    import openfdcm_amd as openfdcm
    maps, _ = openfdcm.score_map(fm, tmpls, window=grid)
    dmaps = np.stack([definition_map(vol, tm, T, grid) for tm in tmpls])
    _assert_same_bits(maps, dmaps, f"score map {grid}")
    pts = _grid_points(grid)
    seam = np.stack(fm.evaluate(tmpls, [pts] * len(tmpls))).reshape(maps.shape)
    _assert_same_bits(seam, dmaps, f"seam {grid}")
    for (rx, ry) in radii:
        ref = peaks_ref(dmaps, max(ks), rx, ry, grid)   # the first k of every template are the first k of the k-max list
        for k in ks:
            want = np.concatenate([ref[ref["tmpl_idx"] == t][:k] for t in range(len(tmpls))])
            if (rx, ry) == (0, 0):
                got = openfdcm.exhaustive_search(fm, tmpls, k=k, window=grid)
            elif k == 1:
                continue
            else:
                got = openfdcm.exhaustive_peaks(fm, tmpls, (rx, ry), k=k, window=grid)
            _same_records(openfdcm.records_of(got), want, f"k {k} radius {rx} {ry} {grid}")
    return dmaps


def _window_checks(fm, tmpls, T, W, H):
    import openfdcm_amd as openfdcm
    boxes = [admissible_box(tm, T, W, H) for tm in tmpls]
    for stride in ((1, 1), (3, 2), (5, 7)):
        want = _window_definition(boxes, stride)
        got = openfdcm.exhaustive_window(fm, tmpls, stride)
        assert got == (want if want is not None else got[:2] + (0, 0) + got[4:]), (stride, got, want)
    return boxes


@pytest.mark.gpu
@pytest.mark.parametrize("via", ["volume", "dt3cpu"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(ADOPTED))
def test_adopted_exhaustive_is_the_definition(via, kind, name):
    """exhaustive_window against the float32 box by brute force; score_map, the seam, top-k (k 1, 8, 64) and peaks (radii
    0, mixed, 32) against the definition on grids that run past every box, strides (1, 1), (3, 2) and (5, 7)."""
    vol, keys, T = adopted(name, kind)
    m, W, H = vol.shape
    fm = device_map(vol, keys, T, via)
    tmpls = adopted_templates(name, 3)
    boxes = _window_checks(fm, tmpls, T, W, H)
    assert any(b is not None for b in boxes)
    orc = O.from_volume(keys, vol, T)
    for stride in ((1, 1), (3, 2), (5, 7)):
        grid = _covering_grid(boxes, stride, 2)
        dmaps = _exhaustive_checks(fm, vol, keys, T, tmpls, grid, radii=((0, 0), (2, 5), (32, 32)) if stride != (1, 1)
                                   else ((0, 0), (1, 0), (2, 5), (32, 32)))
        if stride == (1, 1):
            pts = _grid_points(grid)
            for t, tm in enumerate(tmpls):   # O.evaluate's bits at every admissible point
                adm = ~np.isnan(dmaps[t].reshape(-1))
                if adm.any():
                    _assert_same_bits(O.evaluate(orc, tm, pts[adm]), dmaps[t].reshape(-1)[adm], f"oracle {name} {t}")


def _pivot_center(tmpls):
    out = np.zeros((len(tmpls), 2), dtype=np.float32)
    for t, a in enumerate(tmpls):
        xs, ys = np.concatenate([a[0], a[2]]), np.concatenate([a[1], a[3]])
        out[t] = [(xs.min() + xs.max()) / f32(2), (ys.min() + ys.max()) / f32(2)]
    return out


def _rotation_checks(fm, vol, keys, T, tmpls, angles, pivot, stride, what):
    import openfdcm_amd as openfdcm
    m, W, H = vol.shape
    cs = np.stack([np.cos(np.asarray(angles, dtype=np.float64)), np.sin(np.asarray(angles, dtype=np.float64))],
                  axis=1).astype(np.float32)
    pv = _pivot_center(tmpls) if isinstance(pivot, str) else pivot
    rot = [[rotate_lines(tm, c, s, *(pv[t] if pv is not None else (0.0, 0.0))) for c, s in cs] for t, tm in enumerate(tmpls)]
    keep = [t for t in range(len(tmpls)) if not any(nearest_bins(r.astype(np.float64), m, 1e-5)[1].any() for r in rot[t])]
    assert len(keep) >= len(tmpls) // 2, what      # a rotated line on a bin boundary has no definite bin: left out
    if len(keep) < len(tmpls):
        tmpls, rot = [tmpls[t] for t in keep], [rot[t] for t in keep]
        pv = pv if pv is None or isinstance(pv, str) else pv[keep]
        pivot = pivot if pivot is None or isinstance(pivot, str) else pivot[keep]
    boxes = [admissible_box(r, T, W, H) for rr in rot for r in rr]
    want_w = _window_definition(boxes, stride)
    got_w = openfdcm.rotation_window(fm, tmpls, angles, stride, pivot=pivot)
    if want_w is None:
        assert got_w[2:4] == (0, 0), (what, got_w)
        return
    assert got_w == want_w, (what, got_w, want_w)
    grid = _covering_grid(boxes, stride, 1)
    assert grid[2] * grid[3] * len(tmpls) * len(angles) < 1e7, grid   # the referees stay quick
    vols, _ = openfdcm.rotation_score_map(fm, tmpls, angles, pivot=pivot, window=grid)
    dvols = np.stack([np.stack([definition_map(vol, r, T, grid) for r in rr]) for rr in rot])
    _assert_same_bits(vols, dvols, f"rotation score map {what}")
    for k, (rx, ry, ra, wrap) in ((1, (0, 0, 0, False)), (8, (0, 0, 0, False)), (64, (1, 2, 1, True)), (8, (32, 32, 2, False)),
                                  (64, (3, 0, 0, True))):
        got = openfdcm.records_of(openfdcm.exhaustive_rotation_search(fm, tmpls, angles, k=k, radius=(rx, ry), angle_radius=ra,
                                                                      wrap=wrap, pivot=pivot, window=grid))
        _same_records(got, rotation_peaks_ref(dvols, cs, pv, k, rx, ry, ra, wrap, grid), f"rotations {what} k {k} {rx} {ry} {ra}")


ROT_MAPS = ["1x37", "5x64", "64x5", "257x31", "31x257", "1030x17", "17x1030"]


@pytest.mark.gpu
@pytest.mark.parametrize("pivot", ["center", "none", "far"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ROT_MAPS)
def test_adopted_rotations_are_the_definition(pivot, kind, name):
    """rotation_window, rotation_score_map and the rotation search (top-k, peaks with and without wrap) against
    rotation_ref's float32 unfused rotation of the templates, scored by the definition."""
    vol, keys, T = adopted(name, kind)
    m, W, H = vol.shape
    fm = device_map(vol, keys, T, "volume")
    rng = np.random.default_rng(W + H + len(pivot))
    tmpls = random_templates(rng, W, H, T, m, [1, 3, 4, 9, 12], span=0.3, margin=1e-3) + rotation_boundary_templates(W, H, T, m)
    angles = [0.0, 0.05, -0.1, 0.4, 3.0]
    pv = {"center": "center", "none": None,
          "far": np.array([[-5000.25 + 10 * t, 12345.5 - 3 * t] for t in range(len(tmpls))], dtype=np.float32)}[pivot]
    if pivot == "far" or (pivot == "none" and np.abs(T).max() > 1000):   # small angles about a far pivot
        angles = [0.0, 1e-4, -2e-4, 3e-4]
    elif pivot == "none":
        angles = [0.0, 0.05, -0.03]
    _rotation_checks(fm, vol, keys, T, tmpls, angles, pv, (1, 1), f"{name} {kind} {pivot}")
    _rotation_checks(fm, vol, keys, T, tmpls[:4], angles, pv if pv is None or isinstance(pv, str) else pv[:4], (3, 2),
                     f"{name} {kind} {pivot} s32")


def rotation_boundary_templates(W, H, T, m, c=np.cos(0.05), s=np.sin(0.05)):
    """Vertical one-line templates whose first end point, rotated by the angle 0.05 about the origin, truncates to another
    pixel column when c x + (-s) y is rounded once (fused) instead of twice: the unfused rotation is the definition.  Found
    among the float32 neighbours of x = (n - (-s) y) / c for integer columns n."""
    c, s = f32(c), f32(s)
    ns = -s
    out = []
    rng = np.random.default_rng(W * H)
    for _ in range(200):
        y = f32(rng.uniform(0.2, 0.8) * (H - 1) - float(T[1]))
        n = np.floor(rng.uniform(0.3, 0.7) * (W - 1)) - float(T[0])
        x0 = f32((n - float(ns * y)) / float(c))
        xs = x0 + np.arange(-64, 65).astype(np.float32) * np.spacing(x0)
        ux = c * xs + ns * y                                                  # float32, unfused
        fx = (np.float64(c) * xs.astype(np.float64) + np.float64(ns * y)).astype(np.float32)   # one rounding
        hit = np.flatnonzero(np.floor(ux) != np.floor(fx))
        if len(hit):
            x = xs[hit[0]]
            t = np.array([x, y, x, y + f32(0.1 * (H - 1))], dtype=np.float32).reshape(4, 1)
            if not nearest_bins(t.astype(np.float64), m, 1e-4)[1].any():
                out.append(t)
                if len(out) == 2:
                    break
    return out


# ------------------------------------------------------------------------------------------------ B. built maps
SQUARE = {"s33": (33, 8, 5, 5.0, 1.0, 11), "s64": (64, 12, 4, 5.0, 1.0, 3), "s97": (97, 25, 7, 50.0, 1.37, 4),
          "s150": (150, 30, 12, 0.0, 1.0, 6), "s300": (300, 60, 7, 5.0, 2.2, 8)}
BUILT = list(SQUARE) + list(EDGE_SCENES)
STRIDED = ["s64", "s150", "w5", "w17", "offset", "axis-odd", "depth180", "s97-l1-c0"]   # also at strides (3, 2), (5, 7)


def built(name, dist):
    from openfdcm_amd import synthetic
    from openfdcm_amd.engine import DeviceFeatureMap
    if name == "s97-l1-c0":
        S, n, depth, _, pad, seed = SQUARE["s97"]
        scene, coeff = synthetic.scene(S, n, seed), 0.0
    elif name in SQUARE:
        S, n, depth, coeff, pad, seed = SQUARE[name]
        scene = synthetic.scene(S, n, seed)
    else:
        scene, depth, coeff, pad = EDGE_SCENES[name]
    dev = DeviceFeatureMap.build(scene, depth=depth, coeff=coeff, padding=pad, distance=dist)
    return dev, dev.volume(), np.array(dev.keys, dtype=np.float32), dev.scene_translation.astype(np.float32)


BUILT_CASES = [pytest.param(n, d, id=f"{n}-{i}") for n in BUILT for d, i in ((O.L2, "l2"), (O.L2_SQUARED, "l2sq"), (O.L1, "l1"))]
BUILT_CASES.append(pytest.param("s97-l1-c0", O.L1, id="s97-l1-c0"))


@pytest.mark.gpu
@pytest.mark.parametrize("name, dist", BUILT_CASES)
def test_built_exhaustive_is_the_definition(name, dist):
    """On built maps of every distance: the window, score_map, the seam, O.evaluate, top-k and peaks against the
    definition on grids past every box at strides (1, 1), (3, 2) and (5, 7).  s97-l1-c0 (L1, coefficient 0): integer
    scores, ties everywhere, the (score, g) order across waves and merges."""
    dev, vol, keys, T = built(name, dist)
    m, W, H = vol.shape
    rng = np.random.default_rng(W * 13 + dist)
    tmpls = random_templates(rng, W, H, T, m, [1, 2, 4, 5, 8, 12, 13, 24], span=0.5)
    boxes = _window_checks(dev, tmpls, T, W, H)
    assert any(b is not None for b in boxes)
    orc = O.from_volume(keys, vol, T)
    strides = ((1, 1), (3, 2), (5, 7)) if name in STRIDED else ((1, 1),)
    for stride in strides:
        grid = _covering_grid(boxes, stride, 2)
        dmaps = _exhaustive_checks(dev, vol, keys, T, tmpls, grid, radii=((0, 0), (1, 3), (32, 32)))
        pts = _grid_points(grid)
        sample = np.random.default_rng(stride[0]).permutation(len(pts))[:400]
        for t, tm in enumerate(tmpls):   # O.evaluate's bits and the float64 rescore on a fixed sample per template
            d = dmaps[t].reshape(-1)[sample]
            adm = ~np.isnan(d)
            if not adm.any():
                continue
            _assert_same_bits(O.evaluate(orc, tm, pts[sample][adm]), d[adm], f"oracle {name} {t}")
            for p, s in zip(pts[sample][adm][:10], d[adm][:10]):
                lines = tm.astype(np.float64) + (np.array([T[0] + p[0], T[1] + p[1]] * 2, dtype=np.float32)
                                                 .astype(np.float64)[:, None])
                r, bound, status = rescore(vol, keys, lines, W, H, max(1e-3, 2 * ulp32(lines)), ulp32(tm))
                if status == "ok":
                    assert abs(float(s) - r) <= bound + 1e-30, (name, float(s), r)
    if name == "s97-l1-c0":   # ties among the 64 best scores of most templates
        tied = [len(np.unique(b)) < len(b) for b in (np.sort(d[~np.isnan(d)])[:64] for d in dmaps)]
        assert sum(tied) >= len(tied) // 2, tied


@pytest.mark.gpu
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("name", BUILT)
def test_built_rotations_are_the_definition(dist, name):
    dev, vol, keys, T = built(name, dist)
    m, W, H = vol.shape
    rng = np.random.default_rng(W * 5 + dist)
    tmpls = random_templates(rng, W, H, T, m, [1, 4, 9, 12], span=0.3)
    _rotation_checks(dev, vol, keys, T, tmpls, [0.0, 0.3, -0.2, 1.7], "center", (2, 1), f"{name} {dist}")
    small = [0.0, 1e-4, -2e-4] if np.abs(T).max() > 1000 else [0.0, 0.01, -0.02]   # about the origin, far off
    _rotation_checks(dev, vol, keys, T, tmpls, small, None, (5, 7), f"{name} {dist} origin")


# ------------------------------------------------------------------------------------------------ C. non-finite data
NONFINITE = ["5x64", "64x5", "257x31", "17x1030"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NONFINITE)
def test_nonfinite_exhaustive_has_no_nan_keys(name):
    """Scattered NaN, +inf, -inf and FLT_MAX pixels: a point whose score is NaN has no key.  Top-k, peaks and rotation
    top-k equal the referees on the definition maps with k above the number of finite points; radius-0 peaks equal the
    top-k; infinite scores are keys and order after every finite one."""
    import openfdcm_amd as openfdcm
    W, H, m, T = ADOPTED[name]
    vol = make_volume("nonfinite", m, W, H, W + H)
    keys, T = definition_keys(m).astype(np.float32), np.array(T, dtype=np.float32)
    fm = device_map(vol, keys, T, "volume")
    rng = np.random.default_rng(m + W)
    tmpls = random_templates(rng, W, H, T, m, [1, 2, 3, 4, 8, 12, 24], span=0.4)
    boxes = [admissible_box(tm, T, W, H) for tm in tmpls]
    grid = _covering_grid(boxes, (1, 1), 2)
    dmaps = _exhaustive_checks(fm, vol, keys, T, tmpls, grid, ks=(1, 8, 64), radii=((0, 0), (1, 2), (32, 32)))
    keyed = (~np.isnan(dmaps)).sum(axis=(1, 2))
    assert keyed[-1] < 64, keyed                                # k above the number of points with a key
    adm = ~np.isnan(np.stack([definition_map(np.zeros_like(vol), tm, T, grid) for tm in tmpls]))
    assert np.isinf(dmaps).any() and np.isnan(dmaps[adm]).any()     # NaN from the data at admissible points
    top = openfdcm.records_of(openfdcm.exhaustive_search(fm, tmpls, k=64, window=grid))
    assert not np.isnan(top["score"]).any() and np.isinf(top["score"]).any()
    for t in np.unique(top["tmpl_idx"]):
        s = top["score"][top["tmpl_idx"] == t]
        assert np.all(s[:-1] <= s[1:])
    _same_records(openfdcm.records_of(openfdcm.exhaustive_peaks(fm, tmpls, 0, k=64, window=grid)), top, "radius 0")
    angles = [0.0, 0.02, -0.03]
    _rotation_checks(fm, vol, keys, T, tmpls[:4], angles, "center", (1, 1), f"{name} nonfinite")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("opt", OPTIMIZERS)
@pytest.mark.parametrize("name", NONFINITE)
def test_nonfinite_search_follows_the_oracle(backend, opt, name):
    """The line-walk search on the same volumes: (device) positionally bit-identical to O.search, NaN equal to NaN, for
    every optimiser; the walk's comparisons and argmin follow the reference's with NaN and +-inf present."""
    W, H, m, T = ADOPTED[name]
    vol = make_volume("nonfinite", m, W, H, W + H)
    keys, T = definition_keys(m).astype(np.float32), np.array(T, dtype=np.float32)
    rng = np.random.default_rng(W * 3 + H)
    scene = _scene_inside(rng, W, H, T, 12)
    tmpls = random_templates(rng, W, H, T, m, [1, 2, 3, 4, 5, 8], span=0.5)
    want = _search_records("oracle", vol, keys, T, None, tmpls, scene, opt)
    assert len(want) > 0
    assert np.isnan(want["score"]).any() or np.isinf(want["score"]).any() or backend == "oracle"
    if backend == "device":
        _same_records(_search_records("device", vol, keys, T, "volume", tmpls, scene, opt), want, name)
