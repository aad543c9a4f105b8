"""GPU tests of the detections by matched fraction (include/fdcm.h, "Detections by matched fraction"): records, footprints
and fractions against the numpy definition (matched_ref.py, then detect_all_ref's threshold and nms_ref's greedy rule) on
cost maps that come from the uncapped score maps of one-line templates (capped_ref.line_cost_maps), never from the new
kernels; caps and gate values taken from the data so that points are gated in every case; the identities of the header;
fdcm_matched_fractions against numpy on fdcm_line_costs' floats; infinite and NaN values; an all-zero volume; the 64-bit
addressing form in a fresh process; degenerate inputs; determinism and the public Python surface."""
import os
import subprocess
import sys

import numpy as np
import pytest

from capped_ref import line_cost_maps
from detect_all_ref import thresholded
from detect_ref import records
from matched_ref import fractions, gated, matched_lengths, need, totals
from nms_ref import footprints, nms_ref
from test_gpu_detect import CS7, DEFAULT, EXPONENTIAL, _same_records, built_pair, ragged  # noqa: F401
from test_gpu_exhaustive_peaks import GRIDS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INF = float("inf")
ONE = f32(1)
WIN = (37, 70)  # grid points of the small windows: partial 16 x 64 sub-tiles on both axes, three sub-tiles across


class World:
    """A template set on a grid with everything the referee needs, computed once: the uncapped cost map of every line, the
    caps tau len_i with tau the median of cost_i / len_i over those maps, the capped handle, and per pair the maps of ML and
    of the fraction."""

    def __init__(self, dev, tmpls, grid, cs=None, pv=None, caps=None):
        from openfdcm_amd.engine import DeviceTemplates
        self.dev, self.tmpls, self.grid, self.cs, self.pv = dev, tmpls, grid, cs, pv
        self.A = 1 if cs is None else len(cs)
        self.plain = DeviceTemplates(tmpls)
        self.lens = [np.array(l, dtype=np.float32) for l in self.plain.line_lengths()]
        cost, self.off = line_cost_maps(dev, tmpls, grid, cs, pv)
        self.cost = cost[:, None] if cs is None else cost  # (lines, A, ny, nx)
        if caps is None:
            flat = np.concatenate(self.lens + [np.zeros(0, dtype=np.float32)])
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = self.cost / flat[:, None, None, None]
            self.tau = f32(np.median(ratio[np.isfinite(ratio)]))
            caps = [(self.tau * l).astype(np.float32) for l in self.lens]
        self.caps = caps
        self.tset = DeviceTemplates(tmpls, line_caps=caps)
        self.tl = totals(self.lens)
        self.tl_pair = np.repeat(self.tl, self.A)
        self.ml = np.zeros((len(tmpls) * self.A, grid[3], grid[2]), dtype=np.float32)
        for t in range(len(tmpls)):
            for a in range(self.A):
                self.ml[t * self.A + a] = matched_lengths(self.cost[self.off[t]:self.off[t + 1], a], caps[t], self.lens[t])
        self.frac = fractions(self.ml, self.tl_pair[:, None, None])
        for a in (self.cost, self.ml, self.frac):
            a.setflags(write=False)

    def of_best(self, maps, pairs):
        """Per grid point the value of the pair the plane holds there (pair 0's where there is none)."""
        p = pairs.reshape(-1)
        return maps.reshape(maps.shape[0], -1)[np.where(p >= 0, p, 0), np.arange(p.size)].reshape(pairs.shape)

    def crossed(self):
        """How many templates have an edge of an admissible box inside the grid: some of its points admissible, some not."""
        n = 0
        for t in range(len(self.tmpls)):
            if self.off[t + 1] > self.off[t]:
                adm = ~np.isnan(self.cost[self.off[t]:self.off[t + 1]]).any(axis=0)
                n += bool(adm.any() and not adm.all())
        return n

    def planes(self, penalty, tau):
        s, p = self.dev.best_map(self.tset, self.grid, self.cs, self.pv, penalty=penalty, tau=tau)
        s.setflags(write=False)
        p.setflags(write=False)
        return s, p

    def boxes(self, margin):
        return footprints(self.tmpls, self.cs, self.pv, margin).reshape(-1, 4)

    def ref(self, scores, pairs, boxes, max_score, md, permille, mm):
        """(records, footprints, fractions, grid indices) by the definition."""
        s, p = gated(scores, pairs, self.of_best(self.ml, pairs), need(mm, self.tl_pair))
        s, p = thresholded(s, p, max_score)
        g, sc, F = nms_ref(s, p, boxes, self.grid, md, permille)
        return records(g, sc, p, self.A, self.cs, self.pv, self.grid), F, self.of_best(self.frac, pairs).reshape(-1)[g], g

    def call(self, mm, max_score=INF, md=96, permille=300, margin=0, penalty=DEFAULT, tau=1.0, tset=None):
        return self.dev.exhaustive_detect_all(self.tset if tset is None else tset, self.grid, self.cs, self.pv, max_score=max_score,
                                              max_detections=md, overlap_permille=permille, margin=margin, penalty=penalty, tau=tau,
                                              boxes=True, min_matched=mm, matched=True)

    def gate_values(self, pairs, scores=None, max_score=INF):
        """0, the median and the maximum of the fraction over S_0, the next float above the maximum, and 1."""
        with np.errstate(invalid="ignore"):
            in_s0 = (pairs >= 0) if scores is None else ((pairs >= 0) & (scores <= f32(max_score)))
        fr = np.sort(self.of_best(self.frac, pairs)[in_s0])
        med, top = f32(fr[len(fr) // 2]), f32(fr[-1])
        return [f32(0), med, top, np.nextafter(top, f32(2)), ONE], in_s0

    def poses(self, pairs, g):
        u = pairs.reshape(-1)[g].astype(np.int64)
        x0, y0, nx, ny, sx, sy = self.grid
        return np.stack([u // self.A, u % self.A, x0 + (g % nx) * sx, y0 + (g // nx) * sy], axis=1).astype(np.int32)


def _edges(dev, tmpls, cs, piv):
    """The median of the left and of the upper edge of the templates' admissible boxes."""
    from openfdcm_amd.engine import DeviceTemplates
    xs, ys = [], []
    for t, tm in enumerate(tmpls):
        if tm.shape[1] == 0:
            continue
        one = DeviceTemplates([tm])
        g = dev.exhaustive_window(one, 1, 1) if cs is None else dev.exhaustive_rotations_window(one, cs, piv[t:t + 1], 1, 1)
        g = g.as_tuple()
        xs.append(g[0])
        ys.append(g[1])
    return int(np.median(xs)), int(np.median(ys))


def _window(dev, tmpls, cs, piv, stride):
    """WIN grid points at the stride, placed across the left and the upper edge of the admissible boxes."""
    ex, ey = _edges(dev, tmpls, cs, piv)
    sx, sy = stride
    return (ex - (WIN[0] // 2) * sx, ey - (WIN[1] // 2) * sy, WIN[0], WIN[1], sx, sy)


def _long_set():
    """One template of 70 lines: more than one round of 64 of anything that blocks by 64."""
    rng = np.random.default_rng(71)
    c = rng.uniform(100, 150, size=2)
    return [(c[:, None] + rng.uniform(-45, 45, size=(2, 140))).astype(np.float32).reshape(4, 70, order="F")]


@pytest.fixture(scope="module")
def worlds(built_pair, ragged):
    scene, dev, orc = built_pair
    tmpls, _, piv = ragged
    sets = {"ragged": (tmpls, None, None), "ragged8": (tmpls[:8], CS7, piv[:8]), "long": (_long_set(), None, None)}
    cache = {}

    def get(name, stride):
        if (name, stride) not in cache:
            tm, cs, pv = sets[name]
            grid = GRIDS[0] if stride == "large" else _window(dev, tm, cs, pv, stride)
            cache[(name, stride)] = World(dev, tm, grid, cs, pv)
        return cache[(name, stride)]
    return get


def _same(got, want):
    rec, box, fr = got
    _same_records(rec, want[0])
    assert box.dtype == np.int32 and box.shape == want[1].shape and np.array_equal(box, want[1])
    assert fr.dtype == np.float32 and fr.shape == want[2].shape and fr.tobytes() == want[2].tobytes()


def _check_values(w, scores, pairs, boxes, values, in_s0, md, permille, margin, penalty, tau, max_score=INF):
    """Every gate value against the referee.  On the referee's own output: the median drops a point of S_0 and keeps two
    detections (where the ungated list has two), the value above the maximum leaves nothing (it is no argument when the maximum is 1: FDCM_EINVAL then)."""
    from openfdcm_amd._capi import FdcmError
    zero, med, top, above, one = values
    counts = []
    for mm in values:
        if mm > 1:
            with pytest.raises(FdcmError):
                w.call(mm, max_score, md, permille, margin, penalty, tau)
            counts.append(None)
            continue
        want = w.ref(scores, pairs, boxes, max_score, md, permille, mm)
        got = w.call(mm, max_score, md, permille, margin, penalty, tau)
        passed = int((gated(scores, pairs, w.of_best(w.ml, pairs), need(mm, w.tl_pair))[1][in_s0] >= 0).sum())
        print("min_matched", mm, "points of S_0", int(in_s0.sum()), "passing", passed, "records", len(got[0]), "referee", len(want[0]))
        _same(got, want)
        counts.append((passed, len(want[0])))
    assert counts[0][0] == int(in_s0.sum())
    # (the median keeps half of S_0, so it keeps two detections by construction where nothing is suppressed, at overlap 1000;
    # at a lower overlap two detections need two footprints the rule lets stand, and the small windows may hold one)
    assert counts[1][0] < counts[0][0] and (counts[1][1] >= 2 or permille < 1000)
    if counts[3] is not None:
        assert counts[3] == (0, 0)
    return counts


@pytest.mark.parametrize("name,stride", [("ragged", (1, 1)), ("ragged", (3, 2)), ("ragged8", (1, 1)), ("ragged8", (3, 2)),
                                         ("long", (1, 1)), ("long", (3, 2))])
def test_detections_against_the_definition(worlds, name, stride):
    """Records, boxes and fractions equal the referee byte for byte at every gate value, penalty, overlap and margin.  The
    window holds points without a candidate (it crosses the boxes' left and upper edges) and, for the ragged sets, several
    winning templates; in the set of one long template no point matches everything, so the value above the maximum is an
    argument and leaves no record."""
    w = worlds(name, stride)
    for penalty, tau in [(DEFAULT, 1.0), (EXPONENTIAL, 1.5), (None, 1.0)]:
        scores, pairs = w.planes(penalty, tau)
        assert (pairs >= 0).sum() > 300 and w.crossed() >= (1 if name == "long" else 3)
        if name == "long":
            assert (pairs[:, 0] < 0).any() and (pairs[0] < 0).any()
        else:
            assert len(np.unique(pairs[pairs >= 0] // w.A)) >= 3
        values, in_s0 = w.gate_values(pairs)
        for permille, margin in [(0, 0), (300, 3), (1000, 0)]:
            counts = _check_values(w, scores, pairs, w.boxes(margin), values, in_s0, 96, permille, margin, penalty, tau)
            if name == "long":
                assert values[2] < 1 and counts[3] == (0, 0)


def test_the_large_grid(worlds):
    """GRIDS[0] (200 x 120), the ragged set without rotations: many sub-tiles, most points inside every box."""
    w = worlds("ragged", "large")
    scores, pairs = w.planes(EXPONENTIAL, 1.5)
    values, in_s0 = w.gate_values(pairs)
    assert _check_values(w, scores, pairs, w.boxes(2), values, in_s0, 128, 300, 2, EXPONENTIAL, 1.5)[1][1] >= 2
    assert (pairs < 0).sum() > 1000


@pytest.mark.parametrize("name,stride", [("ragged", (1, 1)), ("ragged8", (3, 2))])
def test_identities(worlds, name, stride):
    w = worlds(name, stride)
    dev, grid, cs, pv = w.dev, w.grid, w.cs, w.pv
    scores, pairs = w.planes(DEFAULT, 1.0)
    values, in_s0 = w.gate_values(pairs)
    med = values[1]
    plain_call = lambda tset, **kw: dev.exhaustive_detect_all(tset, grid, cs, pv, penalty=DEFAULT, boxes=True, **kw)
    # min_matched = 0, and None with the fractions asked for: detect_all's records and boxes
    for permille, margin, md in [(300, 1, 96), (0, 0, 7), (1000, 0, 200)]:
        want = plain_call(w.tset, max_detections=md, overlap_permille=permille, margin=margin)
        for mm in (0.0, None):
            got = plain_call(w.tset, max_detections=md, overlap_permille=permille, margin=margin, min_matched=mm, matched=True)
            assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and len(got[2]) == len(want[0])
        got = plain_call(w.tset, max_detections=md, overlap_permille=permille, margin=margin, min_matched=0.0)
        assert len(got) == 2 and got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
    # a set without caps on a finite volume: frac = 1 everywhere, any min_matched gives detect_all's bytes
    want = plain_call(w.plain, max_detections=96, overlap_permille=300)
    for mm in (0.3, float(med), 1.0):
        got = plain_call(w.plain, max_detections=96, overlap_permille=300, min_matched=mm, matched=True)
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
        assert len(got[2]) == len(want[0]) > 1 and np.all(got[2] == 1)
    # at a fixed min_matched the records of any max_score are the leading ones of the +inf list
    L = w.call(med, md=96, permille=300)
    assert len(L[0]) >= 2 and np.all(np.diff(L[0]["score"]) >= 0)
    for j in (0, len(L[0]) // 2, len(L[0]) - 1):
        s = f32(L[0]["score"][j])
        for ms in (s, np.nextafter(s, f32(-1))):
            if ms < 0:
                continue
            got = w.call(med, max_score=ms, md=96, permille=300)
            n = int((L[0]["score"] <= ms).sum())
            assert len(got[0]) == n and all(a[:n].tobytes() == b.tobytes() for a, b in zip(L, got))
            _same(got, w.ref(scores, pairs, w.boxes(0), ms, 96, 300, med)[:3])
    # overlap 1000, the list not cut: the min_matched = 0 list without the failing points, order kept
    every = w.call(0.0, md=4096, permille=1000)
    assert len(every[0]) == int((pairs >= 0).sum()) < 4096
    want = w.ref(scores, pairs, w.boxes(0), INF, 4096, 1000, 0.0)
    _same(every, want[:3])
    g = want[3]
    for mm in (med, values[2], ONE):
        keep = w.of_best(w.ml, pairs).reshape(-1)[g] >= need(mm, w.tl_pair)[pairs.reshape(-1)[g]]
        got = w.call(mm, md=4096, permille=1000)
        assert 0 < keep.sum() < len(keep) or mm != med
        assert all(a[keep].tobytes() == b.tobytes() for a, b in zip(every, got))
    # the fraction of record l is the pose call's for the record's pose, and the referee's
    poses = w.poses(pairs, g)
    fr = dev.matched_fractions(w.tset, poses, cs, pv)
    assert fr.tobytes() == every[2].tobytes() == w.of_best(w.frac, pairs).reshape(-1)[g].tobytes()
    # two runs of the same call give the same bytes
    again = w.call(med, md=96, permille=300)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(L, again))
    assert dev.matched_fractions(w.tset, poses, cs, pv).tobytes() == fr.tobytes()


@pytest.mark.parametrize("name,stride", [("ragged", (1, 1)), ("ragged8", (1, 1)), ("long", (1, 1))])
def test_matched_fractions_of_pose_lists(worlds, name, stride):
    """Random poses inside and around the window, duplicates, poses far outside the map and, in the ragged sets, the template
    without lines: NaN exactly where fdcm_line_costs says "not admissible", 1 for the template without lines, and elsewhere
    bit for bit the fraction numpy makes of fdcm_line_costs' floats, the caps and the lengths; inside the window also the
    referee's maps."""
    w = worlds(name, stride)
    dev, cs, pv = w.dev, w.cs, w.pv
    T = len(w.tmpls)
    rng = np.random.default_rng(5)
    x0, y0, nx, ny, sx, sy = w.grid
    n = 600
    i, j = rng.integers(0, nx, n), rng.integers(0, ny, n)
    poses = np.stack([rng.integers(0, T, n), rng.integers(0, w.A, n), x0 + i * sx, y0 + j * sy], axis=1).astype(np.int32)
    around = poses[:80].copy()
    around[:, 2:] += rng.integers(-400, 400, (80, 2)).astype(np.int32)
    far = np.array([[T - 1, 0, 9000, 0], [T - 1, w.A - 1, 0, -(1 << 24) + 1], [T - 1, 0, (1 << 24) - 1, 5]], dtype=np.int32)
    everything = np.concatenate([poses, around, far, poses[:50], poses[:1], poses[:1]])
    fr = dev.matched_fractions(w.tset, everything, cs, pv)
    assert fr.dtype == np.float32 and fr.shape == (len(everything),)
    cost, off = dev.line_costs(w.tset, everything, cs, pv)
    want = np.zeros(len(everything), dtype=np.float32)
    for q, (t, a, x, y) in enumerate(everything):
        c = cost[off[q]:off[q + 1]]
        if len(c) == 0:
            want[q] = 1  # no lines: admissible everywhere, TL = 0
        elif np.isnan(c).all():
            want[q] = np.nan
        else:
            want[q] = fractions(matched_lengths(c[:, None], w.caps[t], w.lens[t]), w.tl[t])[0]
    assert fr.tobytes() == want.tobytes()
    inside = w.frac.reshape(len(w.frac), -1)[poses[:, 0] * w.A + poses[:, 1], j * nx + i]
    adm = ~np.isnan(want[:n])
    assert fr[:n][adm].tobytes() == inside[adm].tobytes()
    assert adm.sum() > 100 and (~adm).sum() > 20 and np.isnan(fr[n + 80:n + 83]).all()
    assert len(np.unique(fr[:n][adm])) > (3 if name != "long" else 10)
    assert fr[n + 83:n + 133].tobytes() == fr[:50].tobytes() and fr[-1].tobytes() == fr[-2].tobytes() == fr[0].tobytes()
    if name != "long":
        assert np.all(fr[everything[:, 0] == 0] == 1) and (everything[:, 0] == 0).sum() > 5
    assert w.tset.matched_totals().tobytes() == w.tl.tobytes() and w.plain.matched_totals().tobytes() == w.tl.tobytes()


def _special_volume():
    """test_gpu_detect_all.test_special_values' volume: +inf in a region and one NaN pixel."""
    rng = np.random.default_rng(3)
    vol = np.cumsum(rng.uniform(0, 2, (2, 48, 56)).astype(np.float32), axis=2).astype(np.float32)
    vol[:, 10:22, 30:44] = np.inf
    vol[0, 35, 12] = np.nan
    return vol


def test_special_values():
    """An adopted volume with infinities and a NaN, caps of 0, finite and +inf: an infinite cost is matched under a cap of
    +inf alone, a NaN cost (NaN, or inf - inf) never, a cap of 0 only at cost 0.  The fractions of every pose of a grid that
    runs past the admissible boxes (admissibility from an all-zero volume of the same shape), and the detections at gate
    values from the data."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    vol = _special_volume()
    keys = np.float32([0.0, 1.5])
    dev = DeviceFeatureMap.from_volume(keys, vol, (0.0, 0.0))
    blank = DeviceFeatureMap.from_volume(keys, np.zeros_like(vol), (0.0, 0.0))
    tmpls = [np.array([[0, 0, 9, 0], [0, 3, 9, 3], [2, 0, 2, 7], [5, 2, 5, 2]], dtype=np.float32).T.copy(),  # the last: length zero
             np.array([[0, 0, 0, 5]] + [[i, i % 3, i + 4, i % 3] for i in range(11)], dtype=np.float32).T.copy(),
             np.zeros((4, 0), dtype=np.float32)]
    caps = [np.float32([6, np.inf, 0, 0]), np.float32([np.inf, 0, 4, 9, np.inf, 2, 0, 12, 5, np.inf, 3, 7]), np.zeros(0, dtype=np.float32)]
    inner = dev.exhaustive_window(DeviceTemplates(tmpls), 1, 1).as_tuple()
    grid = (inner[0] - 3, inner[1] - 2, inner[2] + 6, inner[3] + 5, 1, 1)
    w = World(dev, tmpls, grid, caps=caps)
    adm = ~np.isnan(blank.score_map(w.plain, grid))  # (T, ny, nx): geometry alone
    adm[2] = True
    assert (~adm[:2]).any() and adm[:2].any()
    seen_inf = seen_nan = seen_zero = 0
    for t in range(2):
        c = w.cost[w.off[t]:w.off[t + 1], 0][:, adm[t]]
        seen_inf += int((np.isinf(c) & np.isinf(caps[t])[:, None]).sum())
        seen_nan += int(np.isnan(c).sum())
        seen_zero += int(((c == 0) & (caps[t] == 0)[:, None]).sum())
    assert seen_inf > 0 and seen_nan > 0 and seen_zero > 0
    x0, y0, nx, ny, _, _ = grid
    jj, ii = np.mgrid[0:ny, 0:nx]
    for t in range(3):
        poses = np.stack([np.full(nx * ny, t), np.zeros(nx * ny, dtype=np.int64), x0 + ii.ravel(), y0 + jj.ravel()], axis=1).astype(np.int32)
        want = np.where(adm[t], w.frac[t], f32(np.nan)).astype(np.float32)
        got = dev.matched_fractions(w.tset, poses).reshape(ny, nx)
        assert got.tobytes() == want.tobytes()
    assert np.all(w.frac[2] == 1)
    scores, pairs = w.planes(DEFAULT, 1.0)
    assert np.isfinite(scores).any() and np.isnan(scores).any()
    values, in_s0 = w.gate_values(pairs)
    boxes = w.boxes(0)
    for permille, md in [(1000, 4096), (300, 64)]:
        for ms in (INF, f32(np.finfo(np.float32).max)):
            for mm in values:
                if mm > 1:
                    continue
                _same(w.call(mm, ms, md, permille), w.ref(scores, pairs, boxes, ms, md, permille, mm)[:3])
    kept = [int((gated(scores, pairs, w.of_best(w.ml, pairs), need(mm, w.tl_pair))[1] >= 0).sum()) for mm in values if mm <= 1]
    print("points with a candidate", int((pairs >= 0).sum()), "passing at", values, kept)
    assert any(0 < k < (pairs >= 0).sum() for k in kept)


def test_all_zero_volume():
    """Every cost is 0, so every line is matched even under caps of 0: every fraction is 1, every gate passes every point,
    and the records are fdcm_search_exhaustive_detect_all's, ties going by grid index."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    dev = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 40, 30), dtype=np.float32), (0.0, 0.0))
    tmpls = [np.array([[2, 3, 10, 12], [5, 5, 6, 20]], dtype=np.float32).T.copy(), np.array([[1, 1, 2, 2]], dtype=np.float32).T.copy(),
             np.array([[4, 4, 4, 4], [7, 2, 7, 2]], dtype=np.float32).T.copy()]  # the last: lines of length zero only
    grid = (-5, -4, 37, 29, 1, 1)
    for tau in (0.0, 2.0, None):
        tset = DeviceTemplates(tmpls, line_caps=tau)
        assert tset.matched_totals()[2] == 0 and np.all(tset.matched_totals()[:2] > 0)
        for permille, md in [(0, 64), (300, 7), (1000, 4096)]:
            want = dev.exhaustive_detect_all(tset, grid, max_score=0.0, max_detections=md, overlap_permille=permille, boxes=True)
            assert len(want[0]) > 2
            for mm in (0.0, 0.5, 1.0):
                got = dev.exhaustive_detect_all(tset, grid, max_score=0.0, max_detections=md, overlap_permille=permille, boxes=True,
                                                min_matched=mm, matched=True)
                assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
                assert len(got[2]) == len(want[0]) and np.all(got[2] == 1)
        rec = dev.exhaustive_detect_all(tset, grid, max_score=0.0, max_detections=4096, overlap_permille=1000, min_matched=1.0)
        g = ((rec["transform"][:, 5] - grid[1]) * grid[2] + (rec["transform"][:, 2] - grid[0])).astype(np.int64)
        assert len(g) > 64 and np.all(np.diff(g) > 0)  # pure grid order
        assert {0, 1} <= set(rec["tmpl_idx"])
    poses = np.int32([[2, 0, 0, 0], [2, 0, -400, 0], [0, 0, 1, 1]])
    assert dev.matched_fractions(tset, poses).tobytes() == np.float32([1, np.nan, 1]).tobytes()  # NaN goes before TL = 0


def _probe(env):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "matched_probe.py")], capture_output=True, text=True, timeout=300,
                         env={**{k: v for k, v in os.environ.items() if not k.startswith("FDCM_MATCHED")}, **env})
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("matched_probe ")][-1].split()
    return line[1], int(line[3]), int(line[5])


def test_flat_addresses_give_the_same_bytes():
    """The 64-bit addressing form of every kernel of the calls, in a fresh process (the switch is read once per process),
    against this process's default form: the same bytes."""
    spec = __import__("importlib.util").util.spec_from_file_location("matched_probe", os.path.join(ROOT, "tools", "matched_probe.py"))
    probe = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    assert not any(k.startswith("FDCM_MATCHED") for k in os.environ)
    default = probe.run()
    assert default[1] > 1000 and default[2] >= 4
    assert _probe({"FDCM_MATCHED_FLAT": "1"}) == default


def test_degenerate_inputs(built_pair, ragged):
    """An empty set, an empty map, a set without lines, a grid without an admissible point: no records, no fractions, and
    nothing written by the pose call where there is nothing to read."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    scene, dev, orc = built_pair
    tmpls, _, piv = ragged
    capped = DeviceTemplates(tmpls, line_caps=3.0)
    empty_map = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    no_lines = DeviceTemplates([np.zeros((4, 0), dtype=np.float32)] * 2)
    far = (5000, 5000, 40, 30, 1, 1)
    for fm, ts, grid, cs, pv in [(dev, DeviceTemplates([]), GRIDS[0], None, None), (empty_map, capped, (0, 0, 5, 4, 1, 1), None, None),
                                 (dev, no_lines, GRIDS[0], CS7[:2], None), (dev, capped, far, CS7, piv), (dev, capped, far, None, None)]:
        for mm in (0.0, 0.5):
            rec, box, fr = fm.exhaustive_detect_all(ts, grid, cs, pv, max_detections=50, boxes=True, min_matched=mm, matched=True)
            assert len(rec) == 0 and box.shape == (0, 4) and fr.shape == (0,) and fr.dtype == np.float32
    poses = np.int32([[1, 0, 0, 0], [3, 0, 5, 5]])
    assert np.all(empty_map.matched_fractions(capped, poses) == 0)  # nothing written
    assert dev.matched_fractions(capped, np.zeros((0, 4), dtype=np.int32)).shape == (0,)
    assert np.all(dev.matched_fractions(no_lines, np.int32([[1, 0, 3, 4], [0, 0, -9000, 1 << 20]])) == 1)
    assert np.isnan(dev.matched_fractions(capped, np.int32([[5, 0, 9000, 9000]]))).all()
    assert DeviceTemplates([]).matched_totals().shape == (0,)
    # a 1 x 1 grid on a point with a candidate
    w = World(dev, tmpls[:8], GRIDS[0])
    scores, pairs = w.planes(DEFAULT, 1.0)
    cand = np.argwhere(pairs >= 0)
    j, i = cand[len(cand) // 2]
    one = World(dev, tmpls[:8], (GRIDS[0][0] + int(i), GRIDS[0][1] + int(j), 1, 1, 1, 1), caps=w.caps)
    s1, p1 = one.planes(DEFAULT, 1.0)
    fr = f32(one.of_best(one.frac, p1)[0, 0])
    assert p1[0, 0] == pairs[j, i] and fr.tobytes() == f32(w.of_best(w.frac, pairs)[j, i]).tobytes()
    for mm in {f32(0), fr, ONE}:
        got = one.call(mm, md=5)
        _same(got, one.ref(s1, p1, one.boxes(0), INF, 5, 300, mm)[:3])


def test_public_api():
    """openfdcm.exhaustive_detect_all with min_matched / return_matched and openfdcm.matched_fractions on a feature map built
    from an image: the engine's calls on the default window, the tuple shapes, and a partly hidden box that the gate tells
    from a whole one."""
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceTemplates
    img = np.full((160, 200), 40, dtype=np.uint8)
    img[30:70, 25:85] = 200    # a 60 x 40 box, whole
    img[90:140, 120:150] = 200  # a 30 x 50 box ..
    img[90:141, 136:151] = 40   # .. with its right half hidden
    box = lambda bw, bh: np.array([(0, 0, bw, 0), (bw, 0, bw, bh), (bw, bh, 0, bh), (0, bh, 0, 0)], dtype=np.float32).T.copy()
    shapes = [box(58, 38), np.zeros((4, 0), dtype=np.float32), box(28, 48)]
    dt3 = fd.build_image_featuremap(img, fd.Dt3CpuParameters(depth=12, dt3Coeff=5.0, distance=fd.L2), threshold=60)
    pen = fd.DefaultPenalty()
    dets, boxes, matched = fd.exhaustive_detect_all(dt3, shapes, np.inf, overlap=0.3, max_detections=16, penalty=pen, line_caps=2.0,
                                                    return_boxes=True, return_matched=True)
    tset = DeviceTemplates(shapes, line_caps=2.0)
    g = fd.exhaustive_window(dt3, shapes)
    raw = dt3._fm.exhaustive_detect_all(tset, g, max_detections=16, overlap_permille=300, penalty=0, boxes=True, matched=True)
    assert isinstance(dets, fd.MatchList) and dets.records().tobytes() == raw[0].tobytes()
    assert np.array_equal(boxes, raw[1]) and matched.tobytes() == raw[2].tobytes() and matched.dtype == np.float32
    plain = fd.exhaustive_detect_all(dt3, shapes, np.inf, overlap=0.3, max_detections=16, penalty=pen, line_caps=2.0)
    assert isinstance(plain, fd.MatchList) and plain.records().tobytes() == dets.records().tobytes()
    d2, m2 = fd.exhaustive_detect_all(dt3, shapes, np.inf, max_detections=16, penalty=pen, line_caps=2.0, return_matched=True)
    assert isinstance(d2, fd.MatchList) and m2.tobytes() == matched.tobytes()
    rec = dets.records()
    poses = np.stack([rec["tmpl_idx"], np.zeros(len(rec), dtype=np.int64), rec["transform"][:, 2], rec["transform"][:, 5]], axis=1)
    assert fd.matched_fractions(dt3, shapes, poses.astype(np.int32), line_caps=2.0).tobytes() == matched.tobytes()
    assert np.all(fd.matched_fractions(dt3, shapes, poses.astype(np.int32)) == 1)  # no caps: everything is matched
    whole = matched[rec["tmpl_idx"] == 0].max()
    hidden = matched[rec["tmpl_idx"] == 2].max()
    print("matched fraction of the whole box", whole, "of the half-hidden box", hidden)
    assert whole > hidden
    mm = float((whole + hidden) / 2)
    gated_dets = fd.exhaustive_detect_all(dt3, shapes, np.inf, max_detections=16, penalty=pen, line_caps=2.0, min_matched=mm)
    assert isinstance(gated_dets, fd.MatchList) and len(gated_dets) >= 1
    assert gated_dets.records().tobytes() == dt3._fm.exhaustive_detect_all(tset, g, max_detections=16, overlap_permille=300, penalty=0,
                                                                           min_matched=mm).tobytes()
    assert gated_dets.records().tobytes() != dets.records().tobytes()
    angled, am = fd.exhaustive_detect_all(dt3, shapes, np.inf, stride=2, angles=np.deg2rad([0, 90]), penalty=pen, line_caps=2.0,
                                          min_matched=0.5, return_matched=True, max_detections=8)
    assert len(angled) == len(am) >= 1 and np.all(am >= 0.5)
    with pytest.raises(fd._capi.FdcmError):
        fd.exhaustive_detect_all(dt3, shapes, 1.0, min_matched=1.5)
    wide = np.array([[-400.0, 0.0, dt3._fm.width + 400.0, 0.0]], dtype=np.float32).T.copy()
    m3, b3, f3 = fd.exhaustive_detect_all(dt3._fm, [wide], 1.0, return_boxes=True, return_matched=True, min_matched=0.2)
    assert len(m3) == 0 and b3.shape == (0, 4) and f3.shape == (0,)
    del dt3
    fd.clear_featuremap_pool()
