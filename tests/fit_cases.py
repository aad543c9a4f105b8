"""The cases the tests of fdcm_matches_fit share (include/fdcm.h, "Match lists: pose fit").  Not collected: the tests import
it.

The planted scenes: an L-shaped polygon of six lines posed at 12 random transforms, each on its own 400 x 400 label image --
every posed edge sampled each half pixel and rounded to the pixel grid with rint, labelled with the line's own bin, plus 300
clutter pixels of random labels -- and a start that is off by up to 1.5 degrees and 2.5 px per axis.  radius 4, bin_tolerance 2,
two iterations.  The error of a transform is the largest distance between its posed polygon corners and the planted ones.

The device world: 96 x 80 labels of a synthetic image's edges with three of the templates drawn in, and a list of 300 records
over templates of 0, 1, 3, 64, 65 and 257 lines (the last two cross the kernel's LDS chunk of 64 lanes and of 256 segments):
near the drawn poses, anywhere, at the map's sides, outside it, with NaN, and with tmpl_idx outside the set.  The closed
polygons of 64 and more lines have windows of more than 2048 pixels (several strips), the short lines one strip."""
import functools

import numpy as np

import edge_ref
import fit_ref as FR
import match_ref as MR
from oracle import pyoracle as P

f32 = np.float32

# ---- the planted scenes
ELL = np.float64([[0, 0], [120, 0], [120, 40], [50, 40], [50, 100], [0, 100]])
SIZE, DEPTH, CLUTTER, POSES = 400, 30, 300, 12
FIT = dict(radius=4, bin_tolerance=2, iterations=2)
MAX_ERROR, MAX_SHARE = 0.25, 0.1     # px after the fit, and of the start's error


def polygon_lines(pts):
    pts = np.asarray(pts, dtype=np.float64)
    return np.concatenate([pts, np.roll(pts, -1, axis=0)], axis=1).T      # (4, N): x1, y1, x2, y2


def matrix(angle, x, y, pivot):
    """A rotation by angle about pivot followed by the translation (x, y), float64."""
    c, s = np.cos(angle), np.sin(angle)
    px, py = pivot
    return np.array([c, -s, px - (c * px - s * py) + x, s, c, py - (s * px + c * py) + y])


def corners(M, pts):
    M = np.asarray(M, dtype=np.float64).reshape(2, 3)
    return pts @ M[:, :2].T + M[:, 2]


def error(M, true, pts=ELL):
    """The largest distance between the corners posed by M and by true."""
    return float(np.sqrt(((corners(M, pts) - corners(true, pts)) ** 2).sum(axis=1)).max())


def draw(labels, lines, keys):
    """The posed lines (4, N) into labels: a sample each half pixel, rint, the line's bin."""
    for i in range(lines.shape[1]):
        x1, y1, x2, y2 = (float(v) for v in lines[:, i])
        k = max(2, int(np.ceil(2 * np.hypot(x2 - x1, y2 - y1))) + 1)
        xs, ys = np.rint(np.linspace(x1, x2, k)).astype(int), np.rint(np.linspace(y1, y2, k)).astype(int)
        ok = (xs >= 0) & (xs < labels.shape[1]) & (ys >= 0) & (ys < labels.shape[0])
        labels[ys[ok], xs[ok]] = P.closest_orientation(keys, lines[:, i].astype(np.float32))


@functools.lru_cache(maxsize=None)
def planted():
    """[(labels, true float64 matrix, start record)] and (keys, templates)."""
    rng = np.random.default_rng(5)
    keys = edge_ref.keys_of(DEPTH)
    tmpl = polygon_lines(ELL).astype(np.float32)
    pivot = (60.0, 50.0)
    out = []
    for _ in range(POSES):
        true = matrix(rng.uniform(-np.pi, np.pi), rng.uniform(130, 150), rng.uniform(130, 150), pivot)
        labels = np.full((SIZE, SIZE), 255, dtype=np.uint8)
        draw(labels, corners(true, polygon_lines(ELL).T.reshape(-1, 2)).reshape(-1, 4).T, keys)
        cy, cx = rng.integers(0, SIZE, CLUTTER), rng.integers(0, SIZE, CLUTTER)
        labels[cy, cx] = rng.integers(0, len(keys), CLUTTER)
        da, dx, dy = np.deg2rad(rng.uniform(-1.5, 1.5)), rng.uniform(-2.5, 2.5), rng.uniform(-2.5, 2.5)
        c, s = np.cos(da), np.sin(da)
        centre = corners(true, np.float64([pivot]))[0]
        R = np.array([[c, -s], [s, c]])
        A = R @ true.reshape(2, 3)[:, :2]
        t = R @ (true.reshape(2, 3)[:, 2] - centre) + centre + [dx, dy]
        start = MR.records([0], [0.0], [[A[0, 0], A[0, 1], t[0], A[1, 0], A[1, 1], t[1]]])
        labels.setflags(write=False)
        out.append((labels, true, start))
    return out, keys, [tmpl]


def planted_fit(k, **kw):
    """The referee's fit of planted case k: (records, info, rms)."""
    cases, keys, tmpls = planted()
    labels, _, start = cases[k]
    return FR.fit(labels, keys, (0, 0), SIZE, SIZE, tmpls, start, **{**FIT, **kw})


# ---- the device world
WIDTH, HEIGHT = 96, 80
WORLDS = {"b0-d30": (0, 30), "b5-d6": (5, 6)}
LINES = (0, 1, 3, 64, 65, 257)
# (radius, bin_tolerance: None for m / 2, iterations, damping); without damping a single line is singular (status 2)
PARAMS = [(0, 0, 1, 1e-3), (1, None, 8, 1e-3), (32, 0, 8, 1e-3), (32, None, 1, 1e-3), (3, 1, 2, 0.0)]


def closed(n, rx, ry, cx, cy):
    """A closed polygon of n lines on an ellipse."""
    a = np.linspace(0, 2 * np.pi, n, endpoint=False)
    return polygon_lines(np.stack([cx + rx * np.cos(a), cy + ry * np.sin(a)], axis=1)).astype(np.float32)


def templates():
    tri = polygon_lines([[0, 0], [40, 6], [14, 30]]).astype(np.float32)
    return [np.zeros((4, 0), dtype=np.float32), np.float32([[0.5], [1.25], [17.0], [9.5]]), tri, closed(64, 27, 25, 27, 25),
            closed(65, 30, 22, 30, 22), closed(257, 26, 27, 26, 27)]


class FitWorld:
    """Labels, frame, templates and the record list; the referee's result per parameter set, computed once."""

    def __init__(self, name, seed=41):
        self.border, self.depth = WORLDS[name]
        self.keys = edge_ref.keys_of(self.depth)
        self.m = len(self.keys)
        self.width, self.height = WIDTH, HEIGHT
        self.W, self.H = WIDTH + 2 * self.border, HEIGHT + 2 * self.border
        self.T = (self.border, self.border)
        self.tmpls = templates()
        self.base = 3 if self.border else 0
        rng = np.random.default_rng(seed)
        labels = edge_ref.edge_labels(edge_ref.synthetic_image(WIDTH, HEIGHT, 3), self.depth, 60).copy()
        drawn = {2: matrix(0.3, 40.0, 30.0, (0, 0)), 3: matrix(0.0, 8.0, 12.0, (0, 0)), 5: matrix(-0.2, 32.0, 22.0, (26, 27)),
                 1: matrix(1.1, 70.0, 10.0, (0, 0))}
        for t, M in drawn.items():
            tm = self.tmpls[t].astype(np.float64)
            draw(labels, np.concatenate([corners(M, tm[:2].T).T, corners(M, tm[2:].T).T]), self.keys)
        labels.setflags(write=False)
        self.labels = labels
        rows = []

        def near(t, count, da, d):
            for _ in range(count):
                a, x, y = rng.uniform(-da, da), rng.uniform(-d, d), rng.uniform(-d, d)
                c, s = np.cos(a), np.sin(a)
                R, M = np.array([[c, -s], [s, c]]), drawn[t].reshape(2, 3)
                pv = corners(drawn[t], np.float64([[20, 15]]))[0]
                A, tr = R @ M[:, :2], R @ (M[:, 2] - pv) + pv + [x, y]
                rows.append((t, [A[0, 0], A[0, 1], tr[0], A[1, 0], A[1, 1], tr[1]]))

        def anywhere(t, count):
            for _ in range(count):
                rows.append((t, list(matrix(rng.uniform(-np.pi, np.pi), rng.uniform(-10, 70), rng.uniform(-10, 55), (20, 15)))))
        near(5, 6, 0.03, 2.0); anywhere(5, 2)                      # 257 lines
        near(3, 14, 0.03, 2.0); anywhere(3, 6)                     # 64 lines
        anywhere(4, 20)                                            # 65 lines, nothing drawn
        near(2, 70, 0.05, 3.0); anywhere(2, 50)                    # 3 lines
        near(1, 60, 0.05, 2.0); anywhere(1, 60)                    # 1 line: a single line never fixes a pose (status 1 or 2)
        rows += [(0, [1, 0, 5.5, 0, 1, 5.25]),                     # the template without lines
                 (2, [1, 0, np.nan, 0, 1, 5.0]), (2, [np.inf, 0, 5, 0, 1, 5.0]),
                 (1, [1, 0, -self.border - 1.5, 0, 1, 3.0]),        # an end point at -1: not admissible
                 (1, [1, 0, -self.border - 1.25, 0, 1, 3.0]),       # inside by a quarter pixel
                 (3, list(matrix(0.0, WIDTH + self.border - 54.5, 12.0, (0, 0)))),   # a polygon a pixel from the right side
                 (3, [1, 0, 8, 0, 1, 12]), (3, [1, 0, 8, 0, 1, 12])]                  # the drawn pose itself, twice
        recs = MR.records([t + self.base for t, _ in rows], rng.uniform(0, 40, len(rows)), [M for _, M in rows])
        bad = MR.records([self.base - 1, self.base + len(self.tmpls), self.base + 1000, -(1 << 31)], [1, 2, 3, 4], [[1, 0, 5, 0, 1, 5]] * 4)
        self.recs = np.concatenate([recs[:100], bad[:2], recs[100:], bad[2:]])
        assert len(self.recs) == 300
        self._ref = {}

    def kw(self, radius, tol, iterations, damping=1e-3):
        return dict(radius=radius, bin_tolerance=self.m // 2 if tol is None else tol, iterations=iterations, damping=damping)

    def ref(self, radius, tol, iterations, damping=1e-3, recs=None, **more):
        """The referee's (records, info, rms) of the list, or of recs."""
        key = (radius, tol, iterations, damping, tuple(sorted(more.items())))
        if recs is None and key in self._ref:
            return self._ref[key]
        out = FR.fit(self.labels, self.keys, self.T, self.W, self.H, self.tmpls, self.recs if recs is None else recs, self.base,
                     **self.kw(radius, tol, iterations, damping), **more)
        if recs is None:
            self._ref[key] = out
        return out


@functools.lru_cache(maxsize=None)
def world(name):
    return FitWorld(name)
