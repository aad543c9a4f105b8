"""GPU tests of the per-line caps and the line costs (include/fdcm.h, "Per-line caps and line costs"): every exhaustive
call on a capped set against the numpy referee (capped_ref.py: the clamp and the Eigen-order sum over cost maps that come
from the uncapped score maps of one-line templates, fed to the referees that take volumes), bit for bit; planted NaN and
inf; sets with all caps +inf or no caps against fdcm_templates_create's; fdcm_search untouched; the Python cache key; and
fdcm_line_costs against the one-line maps and against the window search's score bits."""
import ctypes as C

import numpy as np
import pytest

from capped_ref import capped_volumes, clamp, eigen_sum0, line_cost_maps
from detect_ref import best_ref, detect_ref, normalised
from peaks_ref import peaks_ref
from rotation_ref import rot_matrix, rotation_peaks_ref
from windows_ref import window_records

pytestmark = pytest.mark.gpu

W, H, M = 64, 96, 6
T0 = (2.5, 1.25)
COUNTS = [0, 1, 3, 4, 7, 8, 9, 12, 17, 33]  # a block of 8, the trailing packet, the scalar tail, alone and together; > kChunk
ALL_INF = 5                                   # the template whose caps are all +inf
ALL_FINITE = 2                                # .. and one whose caps are the three quantiles
EXPONENTIAL = 1
INF = np.float32(np.inf)
f32 = np.float32


def _keys(depth):
    return np.unique(np.array([f32(f32(f32(i) * f32(np.pi)) / f32(depth)) - f32(np.pi / 2) for i in range(depth)], np.float32))


def _templates(rng, counts):
    """Lines inside a box of at most 24 x 24 px whose size and origin differ per template."""
    out = []
    for n in counts:
        o, ext = rng.uniform(0, 4, size=2), rng.uniform(12, 20, size=2)
        pts = o[:, None] + rng.uniform(0, 1, size=(2, 2 * n)) * ext[:, None]
        out.append(pts.astype(np.float32).reshape(4, n, order="F"))
    return out


def _centers(tmpls):
    out = np.zeros((len(tmpls), 2), dtype=np.float32)
    for t, tm in enumerate(tmpls):
        if tm.shape[1]:
            xs, ys = np.concatenate([tm[0], tm[2]]), np.concatenate([tm[1], tm[3]])
            out[t] = [(xs.min() + xs.max()) / f32(2), (ys.min() + ys.max()) / f32(2)]
    return out


def _cs():
    a = np.deg2rad([0.0, 50.0, 200.0])
    cs = np.stack([np.cos(a), np.sin(a)], axis=1)
    cs[2] *= 1.25  # a rotation with scale: norm != 1
    return cs.astype(np.float32)


CS3 = _cs()


class World:
    """The maps, templates, caps and grids of the module, and the referee's volumes, each computed once and left unchanged."""

    def __init__(self):
        from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
        rng = np.random.default_rng(1807)
        vol = rng.uniform(0.5, 60.0, size=(M, W, H)).astype(np.float32)
        planted = vol.copy()
        planted[:, 20, 30] = np.nan
        planted[:, 41, 66] = np.inf
        self.maps = {"plain": DeviceFeatureMap.from_volume(_keys(M), vol, T0),
                     "planted": DeviceFeatureMap.from_volume(_keys(M), planted, T0)}
        self.tmpls = _templates(rng, COUNTS + [70])  # the eleventh, of 70 lines, is the line costs' alone
        self.piv = _centers(self.tmpls) + f32(0.5)
        self.plain = {10: DeviceTemplates(self.tmpls[:10]), 11: DeviceTemplates(self.tmpls)}
        dev = self.maps["plain"]
        self.grid = dev.exhaustive_window(self.plain[10], 1, 1).as_tuple()
        self.rgrid = dev.exhaustive_rotations_window(self.plain[11], CS3, self.piv, 1, 1).as_tuple()
        x0, y0, nx, ny, _, _ = self.grid
        self.strided = (x0 - 4, y0 - 5, nx // 2 + 6, ny // 3 + 5, 2, 3)  # partly outside every box
        self._cache = {}
        # caps: per line 0, +inf or a quantile of its own cost over the template's admissible points
        cost, off, unc = self.costs("plain", self.grid, False)
        self.caps = []
        for t in range(11):
            adm = ~np.isnan(unc[t])
            c = np.full(off[t + 1] - off[t], INF, dtype=np.float32)
            for i in range(len(c)):
                kind = 2 + i % 3 if t == ALL_FINITE else rng.choice(5, p=[0.12, 0.13, 0.25, 0.25, 0.25])
                if t != ALL_INF and kind != 1:
                    c[i] = 0 if kind == 0 else np.quantile(cost[off[t] + i][adm], [0.25, 0.5, 0.75][kind - 2]).astype(np.float32)
            self.caps.append(c)
        self.capped = {10: DeviceTemplates(self.tmpls[:10], line_caps=self.caps[:10]), 11: DeviceTemplates(self.tmpls, line_caps=self.caps)}

    def costs(self, which, grid, rot):
        """(cost maps of the 164 lines, offsets, the 11 templates' uncapped maps) of a map on a grid, with CS3 or without."""
        key = (which, grid, rot)
        if key not in self._cache:
            dev = self.maps[which]
            cost, off = line_cost_maps(dev, self.tmpls, grid, CS3 if rot else None, self.piv if rot else None)
            unc = dev.rotation_score_map(self.plain[11], grid, CS3, self.piv) if rot else dev.score_map(self.plain[11], grid)
            for a in (cost, unc):
                a.setflags(write=False)
            self._cache[key] = (cost, off, unc)
        return self._cache[key]

    def ref(self, which, grid, rot, nt=10, caps=None):
        """The referee's capped volumes of the first nt templates: (nt, ny, nx), or (nt, 3, ny, nx) with rotations."""
        cost, off, unc = self.costs(which, grid, rot)
        v = capped_volumes(cost[:off[nt]], off[:nt + 1], (caps or self.caps)[:nt], unc[:nt])
        v.setflags(write=False)
        return v


@pytest.fixture(scope="module")
def world():
    return World()


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()  # NaN is the one quiet NaN on both sides


def _same_records(got, want):
    assert len(got) == len(want)
    assert np.array_equal(got["tmpl_idx"], want["tmpl_idx"])
    assert got.tobytes() == want.tobytes()


def test_inputs_exercise_both_branches_of_the_clamp(world):
    """A check of the inputs, not of the device: over the lines with finite non-zero caps between 20 % and 80 % of the
    admissible (line, point) pairs exceed their cap; caps of 0 and +inf both occur; the default window spans more than one
    16 x 64 sub-tile on both axes with partial tiles."""
    cost, off, unc = world.costs("plain", world.grid, False)
    over = total = 0
    for t in range(10):
        adm = ~np.isnan(unc[t])
        for i, c in enumerate(world.caps[t]):
            if 0 < c < INF:
                v = cost[off[t] + i][adm]
                over += int((v > c).sum())
                total += v.size
    assert total > 10000 and 0.2 < over / total < 0.8
    flat = np.concatenate(world.caps[:10])
    assert (flat == 0).sum() >= 3 and np.isinf(flat).sum() >= 3 + COUNTS[ALL_INF] and np.isinf(world.caps[ALL_INF]).all()
    x0, y0, nx, ny, sx, sy = world.grid
    assert nx > 16 and nx % 16 and ny > 64 and ny % 64 and (sx, sy) == (1, 1)
    assert [t.shape[1] for t in world.tmpls[:10]] == COUNTS
    for t in world.tmpls:
        if t.shape[1]:
            assert max(t[[0, 2]].max() - t[[0, 2]].min(), t[[1, 3]].max() - t[[1, 3]].min()) <= 24


@pytest.mark.parametrize("which", ["plain", "planted"])
@pytest.mark.parametrize("grid", ["default", "strided"])
def test_score_map(world, which, grid):
    g = world.grid if grid == "default" else world.strided
    want = world.ref(which, g, False)
    got = world.maps[which].score_map(world.capped[10], g)
    assert _same_bits(got, want)
    unc = world.costs(which, g, False)[2][:10]
    assert not _same_bits(got, unc) and _same_bits(got[ALL_INF], unc[ALL_INF]) and _same_bits(got[0], unc[0])
    assert np.isnan(got).any() and (~np.isnan(got)).sum() > 4000


@pytest.mark.parametrize("which", ["plain", "planted"])
def test_search_and_peaks(world, which):
    dev, tset = world.maps[which], world.capped[10]
    for g in (world.grid, world.strided):
        maps = world.ref(which, g, False)
        for k in (1, 8):
            _same_records(dev.exhaustive_search(tset, g, k=k), peaks_ref(maps, k, 0, 0, g, skip={0}))
        _same_records(dev.exhaustive_peaks(tset, g, k=8, rx=2, ry=2, tmpl_index_base=3), peaks_ref(maps, 8, 2, 2, g, base=3, skip={0}))


@pytest.mark.parametrize("which", ["plain", "planted"])
def test_rotations(world, which):
    """Three rotations, one with scale, explicit pivots: a line keeps its cap under each."""
    dev, tset = world.maps[which], world.capped[10]
    g, piv = world.rgrid, world.piv[:10]
    vols = world.ref(which, g, True)
    assert _same_bits(dev.rotation_score_map(tset, g, CS3, piv), vols)
    assert not _same_bits(vols, world.costs(which, g, True)[2][:10])
    for k, rx, ry, ra, wrap in [(8, 0, 0, 0, False), (8, 2, 2, 1, True), (1, 2, 1, 1, False)]:
        got = dev.exhaustive_rotation_search(tset, g, CS3, piv, k=k, rx=rx, ry=ry, ra=ra, wrap=wrap)
        _same_records(got, rotation_peaks_ref(vols, CS3, piv, k, rx, ry, ra, wrap, g, skip={0}))
        assert len(got) >= 9 * min(k, 2)


def test_window_search(world):
    """A handful of jobs, one of them a wrapped run, at stride 1 and at stride (2, 3); and translations only."""
    dev, tset = world.maps["plain"], world.capped[10]
    X0, Y0, NX, NY, _, _ = world.rgrid
    vols = world.ref("plain", world.rgrid, True)
    per_t = [None if COUNTS[t] == 0 else vols[t] for t in range(10)]
    jobs = np.array([(3, 0, 3, X0 + 2, Y0 + 3, 9, 11), (9, 2, 2, X0 + 10, Y0 + 20, 7, 5), (0, 0, 1, X0, Y0, 4, 4),
                     (4, 1, 1, X0, Y0, NX // 3, NY // 3), (7, 1, 3, X0 + NX // 2, Y0 + NY // 2, 5, 6), (5, 2, 1, X0 + 20, Y0 + 30, 3, 3)],
                    dtype=np.int32)
    for sx, sy in [(1, 1), (2, 3)]:
        for k in (1, 5):
            got = dev.exhaustive_window_search(tset, jobs, CS3, world.piv[:10], sx=sx, sy=sy, wrap=True, k=k)
            want = window_records(per_t, (X0, Y0, NX, NY), jobs, CS3, world.piv[:10], k, sx, sy, True)
            _same_records(got[0], want[0])
            assert np.array_equal(got[1], want[1]) and len(got[0]) > 4
    x0, y0, nx, ny, _, _ = world.grid
    maps = world.ref("plain", world.grid, False)
    per_t = [None if COUNTS[t] == 0 else maps[t][None] for t in range(10)]
    jobs = np.array([(9, 0, 1, x0 + 3, y0 + 5, 8, 20), (2, 0, 1, x0, y0, nx, 9), (8, 0, 1, x0 + 11, y0 + 40, 1, 1)], dtype=np.int32)
    got = dev.exhaustive_window_search(tset, jobs, k=5)
    want = window_records(per_t, (x0, y0, nx, ny), jobs, None, None, 5, 1, 1, False)
    _same_records(got[0], want[0])
    assert np.array_equal(got[1], want[1])


@pytest.mark.parametrize("which", ["plain", "planted"])
@pytest.mark.parametrize("rot", [False, True])
def test_best_map_and_detections(world, which, rot):
    """ExponentialPenalty(1.5): the denominators do not look at caps; more than kChunk templates, so two chunks merge."""
    dev, tset = world.maps[which], world.capped[10]
    g = world.rgrid if rot else world.grid
    cs, piv = (CS3, world.piv[:10]) if rot else (None, None)
    vols = world.ref(which, g, rot)
    q = normalised(vols if rot else vols[:, None], world.plain[10].lengths(), EXPONENTIAL, 1.5)
    assert np.array_equal(tset.lengths(), world.plain[10].lengths())
    want = best_ref(q, skip={0})
    got = dev.best_map(tset, g, cs, piv, penalty=EXPONENTIAL, tau=1.5)
    assert np.array_equal(got[1], want[1]) and _same_bits(got[0], want[0])
    assert len(np.unique(got[1][got[1] >= 0] // q.shape[1])) >= 3
    for k, rx, ry in [(8, 2, 2), (1, 0, 0)]:
        _same_records(dev.exhaustive_detect(tset, g, cs, piv, k=k, rx=rx, ry=ry, penalty=EXPONENTIAL, tau=1.5),
                      detect_ref(q, k, rx, ry, g, cs=cs, pivots=piv, skip={0}))


def test_planted_nan_and_inf(world):
    """On the referee's data: the planted NaN makes admissible points NaN (they have no key: the records above equal the
    referee's, which leaves them out); the planted inf is a cost of +inf that a finite cap replaces and +inf keeps."""
    cost, off, unc = world.costs("planted", world.grid, False)
    plain = world.costs("plain", world.grid, False)[2]
    ref = world.ref("planted", world.grid, False)
    nan_pts = np.isnan(ref) & ~np.isnan(plain[:10])
    assert nan_pts.sum() > 50 and nan_pts[1:].any(axis=(1, 2)).all()
    dev, tset = world.maps["planted"], world.capped[10]
    got = dev.score_map(tset, world.grid)
    assert np.isnan(got[nan_pts]).all()
    rec = dev.exhaustive_search(tset, world.grid, k=64)
    x0, y0, nx, ny, _, _ = world.grid
    i, j = (rec["transform"][:, 2] - x0).astype(int), (rec["transform"][:, 5] - y0).astype(int)
    assert not nan_pts[rec["tmpl_idx"], j, i].any() and not np.isnan(rec["score"]).any()
    seen_cap = seen_inf = 0
    for t in range(1, 10):
        for l, c in enumerate(world.caps[t]):
            at = np.isinf(cost[off[t] + l]) & ~np.isnan(unc[t])  # (at most one point per end of the line)
            capped = clamp(cost[off[t] + l], c)[at]
            assert np.all(capped == c)
            seen_cap += int(at.any() and c < INF)
            seen_inf += int(at.any() and c == INF)
    assert seen_cap > 20 and seen_inf > 8
    assert np.isinf(unc[ALL_INF]).any() and _same_bits(got[ALL_INF], unc[ALL_INF])
    all_finite = [t for t in range(1, 10) if np.all(world.caps[t] < INF)]
    assert ALL_FINITE in all_finite and all(np.isinf(unc[t]).any() and not np.isinf(got[t]).any() for t in all_finite)


def _null_capped(tmpls):
    """A set made by fdcm_templates_create_capped with caps = NULL."""
    from openfdcm_amd import _capi as capi
    from openfdcm_amd.engine import DeviceTemplates
    flat, offsets = capi.pack_templates(tmpls)
    h = C.c_void_p()
    capi.check(capi.lib().fdcm_templates_create_capped(capi.fptr(flat), offsets.ctypes.data_as(C.POINTER(C.c_int64)), len(tmpls), None,
                                                       C.byref(h)))
    ts = DeviceTemplates.__new__(DeviceTemplates)
    ts.count, ts.n_lines, ts._h, ts._offsets = len(tmpls), int(offsets[-1]), h, offsets
    return ts


def test_infinite_and_absent_caps_change_nothing(world):
    """All caps +inf, and caps = NULL, give the bytes of fdcm_templates_create's set in every call above."""
    from openfdcm_amd.engine import DeviceTemplates
    tm = world.tmpls[:10]
    base = world.plain[10]
    sets = [DeviceTemplates(tm, line_caps=[np.full(n, INF, dtype=np.float32) for n in COUNTS]), _null_capped(tm)]
    for ts in sets:
        assert all(np.isinf(c).all() for c in ts.line_caps()) and [len(c) for c in ts.line_caps()] == COUNTS
    assert all(np.isinf(c).all() for c in base.line_caps())
    X0, Y0, NX, NY, _, _ = world.rgrid
    jobs = np.array([(3, 0, 3, X0 + 2, Y0 + 3, 9, 11), (9, 2, 2, X0 + 10, Y0 + 20, 7, 5)], dtype=np.int32)
    piv = world.piv[:10]

    def calls(dev, ts):
        out = [dev.score_map(ts, world.grid), dev.score_map(ts, world.strided), dev.exhaustive_search(ts, world.grid, k=8),
               dev.exhaustive_peaks(ts, world.grid, k=8, rx=2, ry=2), dev.rotation_score_map(ts, world.rgrid, CS3, piv),
               dev.exhaustive_rotation_search(ts, world.rgrid, CS3, piv, k=8, rx=2, ry=2, ra=1, wrap=True),
               *dev.exhaustive_window_search(ts, jobs, CS3, piv, wrap=True, k=5),
               *dev.best_map(ts, world.grid, penalty=EXPONENTIAL, tau=1.5), *dev.best_map(ts, world.rgrid, CS3, piv, penalty=EXPONENTIAL, tau=1.5),
               dev.exhaustive_detect(ts, world.grid, k=8, rx=2, ry=2, penalty=EXPONENTIAL, tau=1.5),
               dev.exhaustive_detect(ts, world.rgrid, CS3, piv, k=8, rx=2, ry=2, penalty=EXPONENTIAL, tau=1.5)]
        return [np.asarray(o).tobytes() for o in out]
    for which in ("plain", "planted"):
        want = calls(world.maps[which], base)
        assert all(len(w) > 0 for w in want)
        for ts in sets:
            assert calls(world.maps[which], ts) == want


def test_reference_search_ignores_caps(world):
    """fdcm_search on the capped set returns the bytes it returns on the uncapped one."""
    from openfdcm_amd.engine import search_raw
    rng = np.random.default_rng(5)
    scene = rng.uniform(4, 56, size=(4, 12)).astype(np.float32)
    dev = world.maps["plain"]
    want = search_raw(dev, world.plain[10], scene, 4, 4, 1, 10)
    got = search_raw(dev, world.capped[10], scene, 4, 4, 1, 10)
    assert len(want) > 0 and got.tobytes() == want.tobytes()
    assert np.array_equal(world.capped[10].lengths(), world.plain[10].lengths())


def test_python_cache_keys_on_the_caps(world):
    """One list used uncapped, with line_caps = tau, and uncapped again: the first and third results are identical and the
    second is the referee's for the caps tau * len_i.  tau = 1 caps a line at its length, a few to 28 px here, and costs are
    |a - b| of values uniform in (0.5, 60), below c with probability 1 - (1 - c / 59.5)^2: both branches of the clamp occur."""
    import openfdcm_amd as fd
    dev = world.maps["plain"]
    tm = list(world.tmpls[:10])
    fd.clear_template_cache()
    first, g = fd.score_map(dev, tm)
    second, g2 = fd.score_map(dev, tm, line_caps=1.0)
    third, g3 = fd.score_map(dev, tm)
    assert g == g2 == g3 == world.grid
    assert first.tobytes() == third.tobytes() and _same_bits(first, world.costs("plain", g, False)[2][:10])
    caps = fd.line_caps(tm, 1.0)
    cost, off, unc = world.costs("plain", g, False)
    over = np.concatenate([(cost[off[t] + i] > c)[~np.isnan(unc[t])] for t in range(10) for i, c in enumerate(caps[t])])
    assert 0.05 < over.mean() < 0.95
    assert _same_bits(second, world.ref("plain", g, False, caps=caps)) and second.tobytes() != first.tobytes()
    # per-template arrays are the same key as the scalar they state; other caps are another
    assert fd.score_map(dev, tm, line_caps=caps)[0].tobytes() == second.tobytes()
    assert _same_bits(fd.score_map(dev, tm, line_caps=world.caps[:10])[0], world.ref("plain", g, False))
    m = fd.exhaustive_search(dev, tm, k=8, line_caps=1.0)
    _same_records(m.records(), peaks_ref(world.ref("plain", g, False, caps=caps), 8, 0, 0, g, skip={0}))
    _same_records(fd.exhaustive_search(dev, tm, k=8).records(), peaks_ref(unc[:10], 8, 0, 0, g, skip={0}))
    with pytest.raises(ValueError):
        fd.score_map(dev, world.plain[10], line_caps=1.0)
    fd.clear_template_cache()


# ---------------------------------------------------------------- line costs
def _poses_of(rec, cs, piv, base=0):
    """(tmpl, a, x, y) of match records: a by the exact (c, s), the translation transform - m rounded."""
    out = np.zeros((len(rec), 4), dtype=np.int32)
    for q, r in enumerate(rec):
        t, tr = int(r["tmpl_idx"]) - base, r["transform"]
        if cs is None:
            out[q] = (t, 0, int(tr[2]), int(tr[5]))
            continue
        a = int(np.flatnonzero((cs[:, 0] == tr[0]) & (cs[:, 1] == tr[3]))[0])
        m = rot_matrix(cs[a, 0], cs[a, 1], piv[t, 0], piv[t, 1])
        out[q] = (t, a, int(np.rint(float(tr[2]) - float(m[0, 2]))), int(np.rint(float(tr[5]) - float(m[1, 2]))))
    return out


def _admissible_points(unc, t, a, grid, count, rng):
    """count poses (t, a, x, y) at random admissible grid points of template t under rotation a (unc: (T, A, ny, nx))."""
    j, i = np.nonzero(~np.isnan(unc[t, a]))
    pick = rng.choice(len(j), size=count, replace=False)
    return [(t, a, grid[0] + int(i[p]), grid[1] + int(j[p])) for p in pick]


@pytest.mark.parametrize("rot", [True, False])
def test_line_costs(world, rot):
    """Poses of the capped detections, poses of the 70-line template (two rounds of the lane loop) and of the template
    without lines, and poses that are not admissible.  Every line's cost is the one-line map's value at the point; clamped
    with the caps and summed in Eigen's order the costs give the window search's score bits; poses that are not admissible
    are NaN throughout."""
    dev, tset = world.maps["plain"], world.capped[11]
    g = world.rgrid if rot else world.grid
    cs, piv = (CS3, world.piv) if rot else (None, None)
    A = 3 if rot else 1
    cost, off, unc = world.costs("plain", g, rot)
    if not rot:
        cost, unc = cost[:, None], unc[:, None]
    rng = np.random.default_rng(77)
    det = dev.exhaustive_detect(tset, g, cs, piv, k=16, rx=2, ry=2, penalty=EXPONENTIAL, tau=1.5)
    assert len(det) >= 8
    good = [tuple(p) for p in _poses_of(det, cs, piv)]
    for a in range(A):
        good += _admissible_points(unc, 10, a, g, 3, rng) + _admissible_points(unc, 0, a, g, 1, rng)
    X0, Y0, NX, NY, _, _ = g
    j, i = np.nonzero(np.isnan(unc[3, A - 1]))  # on the grid, outside template 3's box
    bad = [(3, A - 1, X0 + int(i[0]), Y0 + int(j[0])), (3, 0, X0 - 50, Y0), (10, A - 1, 5000, 5000), (4, 0, -(1 << 24) + 1, 0),
           (9, 0, 0, (1 << 24) - 1)]
    poses = np.array(good + bad, dtype=np.int32)
    flat, offsets = dev.line_costs(tset, poses, cs, piv)
    n_lines = np.array([world.tmpls[t].shape[1] for t in poses[:, 0]])
    assert flat.dtype == np.float32 and offsets.dtype == np.int64
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(n_lines)])) and len(flat) == offsets[-1]
    assert 70 in n_lines and 0 in n_lines
    # the window search's answer for the one-point jobs of the same poses
    jobs = np.array([(t, a, 1, x, y, 1, 1) for t, a, x, y in poses], dtype=np.int32)
    rec, joff = dev.exhaustive_window_search(tset, jobs, cs, piv, k=1)
    scored = 0
    for q, (t, a, x, y) in enumerate(poses):
        mine = flat[offsets[q]:offsets[q + 1]]
        if q < len(good):
            want = cost[off[t]:off[t + 1], a, y - Y0, x - X0]
            assert _same_bits(mine, want), (q, t, a, x, y)
            assert not np.isnan(mine).any()
        else:
            assert np.isnan(mine).all() and len(mine) == n_lines[q] > 0, q
        total = eigen_sum0(clamp(mine, world.caps[t]))
        r = rec[joff[q]:joff[q + 1]]
        if q < len(good) and n_lines[q]:
            assert len(r) == 1 and _same_bits(r["score"][0], total), (q, t, a, x, y)
            scored += 1
            if not rot and q < 3:  # rot == NULL: fdcm_search_exhaustive on the one-point grid
                from openfdcm_amd.engine import DeviceTemplates
                one = DeviceTemplates([world.tmpls[t]], line_caps=[world.caps[t]])
                assert _same_bits(dev.exhaustive_search(one, (x, y, 1, 1, 1, 1), k=1)["score"], [total])
        else:
            assert len(r) == 0
    assert scored >= 8 + 3 * A
    # the clamp matters for these poses: the capped sums differ from the plain ones somewhere
    plain_sums = [eigen_sum0(flat[offsets[q]:offsets[q + 1]]) for q in range(len(good))]
    capped_sums = [eigen_sum0(clamp(flat[offsets[q]:offsets[q + 1]], world.caps[poses[q, 0]])) for q in range(len(good))]
    assert not _same_bits(plain_sums, capped_sums)
    # an uncapped set gives the same costs: the output is uncapped
    again = dev.line_costs(world.plain[11], poses, cs, piv)
    assert _same_bits(again[0], flat) and np.array_equal(again[1], offsets)


def test_line_costs_empty_inputs_and_handle_checks(world):
    from openfdcm_amd import _capi as capi
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    dev, tset = world.maps["plain"], world.capped[11]
    flat, offsets = dev.line_costs(tset, np.zeros((0, 4), dtype=np.int32))
    assert len(flat) == 0 and offsets.tolist() == [0]
    poses = np.array([(3, 0, 5, 5), (10, 0, 6, 6)], dtype=np.int32)
    empty = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    for fm, ts in [(empty, tset), (dev, DeviceTemplates([]))]:
        flat, offsets = fm.line_costs(ts, poses)
        assert len(flat) == 0 and offsets.tolist() == [0, 0, 0]
    flat, offsets = dev.line_costs(tset, np.array([(0, 0, 5, 5)], dtype=np.int32))  # a template without lines: no floats
    assert len(flat) == 0 and offsets.tolist() == [0, 0]
    for bad, what in [((11, 0, 5, 5), "tmpl is outside"), ((3, 1, 5, 5), "a must be 0")]:
        with pytest.raises(capi.FdcmError, match=what):
            dev.line_costs(tset, np.array([poses[0], bad], dtype=np.int32))
    bad_piv = world.piv.copy()
    bad_piv[2, 0] = np.nan
    with pytest.raises(capi.FdcmError, match="pivots"):
        dev.line_costs(tset, poses, CS3, bad_piv)
    want = dev.line_costs(tset, poses)
    assert len(want[0]) == 4 + 70 and not np.isnan(want[0]).any()


def test_public_line_costs_from_detections(world):
    """openfdcm.line_costs on the poses pose_windows(records, angles, angles, pivots, 0, 0, 0)[:, [0, 1, 3, 4]] makes of
    capped detections equals the engine call, and the matched fraction is a number in [0, 1]."""
    import openfdcm_amd as fd
    dev = world.maps["plain"]
    tm = list(world.tmpls)
    angles = np.deg2rad([0.0, 35.0, 180.0])
    fd.clear_template_cache()
    det = fd.exhaustive_detect(dev, tm, radius=2, k=8, penalty=fd.ExponentialPenalty(1.5), angles=angles, line_caps=world.caps)
    assert len(det) >= 4
    piv = fd.template_pivots(tm)
    poses = fd.pose_windows(det, angles, angles, piv, 0, 0, 0)[:, [0, 1, 3, 4]]
    flat, offsets = fd.line_costs(dev, tm, poses, angles=angles)
    cs = np.stack([np.cos(angles), np.sin(angles)], axis=1).astype(np.float32)
    want = dev.line_costs(world.plain[11], poses, cs, piv)
    assert _same_bits(flat, want[0]) and np.array_equal(offsets, want[1]) and not np.isnan(flat).any()
    lens = fd.DeviceTemplates(tm).line_lengths()
    for q, (t, a, x, y) in enumerate(poses):
        c = flat[offsets[q]:offsets[q + 1]]
        frac = lens[t][c <= world.caps[t]].sum() / lens[t].sum()
        assert 0.0 <= frac <= 1.0
        # the detection's score is the capped sum, normalised
        total = eigen_sum0(clamp(c, world.caps[t]))
        q_want = normalised(np.float32([[[[total]]]]), [fd.get_template_lengths(tm)[t]], EXPONENTIAL, 1.5)[0, 0, 0, 0]
        assert _same_bits(det.records()["score"][q], q_want)
    d0 = fd.exhaustive_detect(dev, tm, radius=2, k=4, line_caps=world.caps)  # without angles: a = 0
    rec = d0.records()
    p0 = np.stack([rec["tmpl_idx"], np.zeros(len(rec), np.int32), rec["transform"][:, 2].astype(np.int32),
                   rec["transform"][:, 5].astype(np.int32)], axis=1)
    f0, o0 = fd.line_costs(dev, tm, p0)
    for q, (t, a, x, y) in enumerate(p0):
        assert _same_bits(rec["score"][q], eigen_sum0(clamp(f0[o0[q]:o0[q + 1]], world.caps[t])))
    fd.clear_template_cache()
