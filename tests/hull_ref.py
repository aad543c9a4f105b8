"""The numpy / Python-integer statement of the hull footprints (include/fdcm.h, "Hull footprints"), the referee of
fdcm_lines_footprint_spans and of the detection calls on a hull set.  Not collected: the tests import it.

  vertices        of a pair: per posed end point (rotation_ref.rotate_lines' float32 rule; without a table the lines as they
                  are) the corners (floor(x) -+ m, floor(y) -+ m), each coordinate clamped to [-2^25, 2^25] after the margin,
                  which is nms_ref.box_of_lines' arithmetic; none for a template without lines or with a NaN end point
  rows_by_pairs   the shape row by row from all ordered vertex pairs in exact rationals: the statement of the header
  rows_by_halfplanes  a second, independent statement: a monotone-chain hull and, per pixel of the box, "no hull edge has the
                  pixel strictly outside" with int cross products
  shapes          per pair u = t A + a its box, rows and area
  span_table      the (row_offsets, spans, areas) fdcm_lines_footprint_spans returns
  hull_objects_nms  the greedy rule over the planes of detect_ref / objects_ref (one plane: G = 1), with both limits
  hull_list_nms   the greedy rule over a list of entries (key, object, box, shape): the windows' calls"""
from fractions import Fraction

import numpy as np

from nms_ref import LIM, box_of_lines
from rotation_ref import rotate_lines


def vertices(lines, margin=0):
    """The set of integer vertices (x, y) of one (4, N) line array; empty for the empty shape."""
    lines = np.asarray(lines, dtype=np.float32).reshape(4, -1)
    if lines.shape[1] == 0 or np.isnan(lines).any():
        return []

    def at(v, d):
        f = int(np.clip(np.floor(np.float64(v)), -2.0 ** 40, 2.0 ** 40))
        return min(max(f + d, -LIM), LIM)
    out = set()
    for x, y in list(zip(lines[0], lines[1])) + list(zip(lines[2], lines[3])):
        for dx in ((-margin, margin) if margin else (0,)):
            for dy in ((-margin, margin) if margin else (0,)):
                out.add((at(x, dx), at(y, dy)))
    return sorted(out)


def _ceil(fr):
    return -((-fr.numerator) // fr.denominator)


def _floor(fr):
    return fr.numerator // fr.denominator


def rows_by_pairs(verts):
    """rows_by_pairs_exact in int64 arrays, a row at a time over all ordered pairs at once: ceil(min x*) is the minimum of
    ceil(x*) and every product stays below 2^55, so nothing is rounded."""
    if not verts:
        return {}
    v = np.array(verts, dtype=np.int64)
    px, py, qx, qy = v[:, 0][:, None], v[:, 1][:, None], v[:, 0][None, :], v[:, 1][None, :]
    dy = qy - py
    out = {}
    for y in range(int(v[:, 1].min()), int(v[:, 1].max()) + 1):
        on = (py <= y) & (y <= qy)
        flat = on & (dy == 0)
        slope = on & (dy != 0)
        d = np.where(slope, dy, 1)
        num = px * d + (qx - px) * (y - py)
        lo = np.where(slope, -((-num) // d), np.where(flat, np.minimum(px, qx), np.int64(2) ** 62))
        hi = np.where(slope, num // d, np.where(flat, np.maximum(px, qx), -np.int64(2) ** 62))
        out[y] = (int(lo.min()), int(hi.max()))
    return out


def rows_by_pairs_exact(verts):
    """{y: (xl, xr)} for every integer y between the least and greatest vertex y; xl > xr: an empty row.  Python integers and
    exact rationals, the header's words."""
    if not verts:
        return {}
    out = {}
    for y in range(min(v[1] for v in verts), max(v[1] for v in verts) + 1):
        xs = []
        for p in verts:
            for q in verts:
                if not p[1] <= y <= q[1]:
                    continue
                if p[1] == q[1]:
                    xs += [Fraction(p[0]), Fraction(q[0])]
                else:
                    xs.append(p[0] + Fraction((q[0] - p[0]) * (y - p[1]), q[1] - p[1]))
        out[y] = (_ceil(min(xs)), _floor(max(xs)))
    return out


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull(verts):
    """Counter-clockwise hull without collinear points (Andrew's monotone chain); one or two points when degenerate."""
    pts = sorted(set(verts))
    if len(pts) < 3:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def rows_by_halfplanes(verts):
    """The same rows from a per-pixel test; asserts that the pixels of a row are one run."""
    if not verts:
        return {}
    h = hull(verts)
    x0, x1 = min(v[0] for v in verts), max(v[0] for v in verts)
    out = {}
    for y in range(min(v[1] for v in verts), max(v[1] for v in verts) + 1):
        inside = [x for x in range(x0, x1 + 1)
                  if all(_cross(h[e], h[(e + 1) % len(h)], (x, y)) >= 0 for e in range(len(h)))
                  and (len(h) > 2 or (min(p[0] for p in h) <= x <= max(p[0] for p in h) and min(p[1] for p in h) <= y <= max(p[1] for p in h)))]
        if inside:
            assert inside == list(range(inside[0], inside[-1] + 1)), "a row is not one run"
            out[y] = (inside[0], inside[-1])
        else:
            out[y] = (1, 0)
    return out


def _same_rows(a, b):
    """Equal as sets of pixels (an empty row is empty whatever its xl > xr)."""
    return a.keys() == b.keys() and all((a[y] == b[y]) or (a[y][0] > a[y][1] and b[y][0] > b[y][1]) for y in a)


class Shape:
    """A pair's shape: box (x0, y0, x1, y1), xl and xr per row of the box in the box's frame ((0, -1): empty), area."""

    def __init__(self, lines, margin=0, statement=rows_by_pairs):
        self.box = tuple(int(v) for v in box_of_lines(lines, margin))
        rows = statement(vertices(lines, margin))
        n = self.box[3] - self.box[1] + 1
        assert len(rows) == max(0, n) and (not rows or (min(rows) == self.box[1] and max(rows) == self.box[3]))
        self.xl = np.zeros(max(0, n), dtype=np.int64)
        self.xr = np.full(max(0, n), -1, dtype=np.int64)
        for y, (l, r) in rows.items():
            if l <= r:
                self.xl[y - self.box[1]], self.xr[y - self.box[1]] = l - self.box[0], r - self.box[0]
        self.area = int(np.maximum(0, self.xr - self.xl + 1).sum())

    def pixels(self, tx=0, ty=0):
        return {(self.box[0] + x + tx, self.box[1] + r + ty) for r in range(len(self.xl)) for x in range(self.xl[r], self.xr[r] + 1)}


def posed(templates, cs=None, pivots=None):
    """The posed line arrays of every pair, [t][a]."""
    out = []
    for t, tm in enumerate(templates):
        tm = np.asarray(tm, dtype=np.float32).reshape(4, -1)
        if cs is None:
            out.append([tm])
            continue
        px, py = (0.0, 0.0) if pivots is None else pivots[t]
        out.append([rotate_lines(tm, c, s, px, py) for c, s in np.asarray(cs, dtype=np.float32).reshape(-1, 2)])
    return out


def shapes(templates, cs=None, pivots=None, margin=0, statement=rows_by_pairs):
    """The flat list of Shape, pair u = t A + a."""
    return [Shape(l, margin, statement) for row in posed(templates, cs, pivots) for l in row]


def span_table(sh):
    """(row_offsets int64 (P + 1), spans int32 (R, 2), areas int64 (P)) of a list of Shape."""
    off = np.zeros(len(sh) + 1, dtype=np.int64)
    for u, s in enumerate(sh):
        off[u + 1] = off[u] + len(s.xl)
    spans = np.zeros((int(off[-1]), 2), dtype=np.int32)
    for u, s in enumerate(sh):
        spans[off[u]:off[u + 1], 0], spans[off[u]:off[u + 1], 1] = s.xl, s.xr
    return off, spans, np.array([s.area for s in sh], dtype=np.int64)


def overlap(S, s_t, D, d_t):
    """I(g, h) of shape S at translation s_t and shape D at d_t: the sum over the common rows."""
    sy0, dy0 = S.box[1] + s_t[1], D.box[1] + d_t[1]
    ya, yb = max(sy0, dy0), min(S.box[3] + s_t[1], D.box[3] + d_t[1])
    sx0, dx0 = S.box[0] + s_t[0], D.box[0] + d_t[0]
    if ya > yb or min(S.box[2] + s_t[0], D.box[2] + d_t[0]) < max(sx0, dx0):  # (a shape lies inside its box)
        return 0
    a = slice(ya - sy0, yb - sy0 + 1)
    b = slice(ya - dy0, yb - dy0 + 1)
    w = np.minimum(S.xr[a] + sx0, D.xr[b] + dx0) - np.maximum(S.xl[a] + sx0, D.xl[b] + dx0) + 1
    return int(np.maximum(0, w).sum())


def _suppressed(S, s_t, D, d_t, limit):
    inter = overlap(S, s_t, D, d_t)
    return 1000 * inter > limit * (S.area + D.area - inter)


def hull_objects_nms(scores, pairs, sh, grid, max_det, permille, cross=None):
    """The detections as (n, 2) int64 rows (object, flat grid index), in the order found.  scores, pairs: (G, ny, nx) planes of
    objects_ref (or (ny, nx) of detect_ref: one object); sh: the Shape of every pair; the order of the entries is (bits of q,
    g, pair), the limit `permille` within an object and `cross` across."""
    scores = np.asarray(scores, dtype=np.float32)
    if scores.ndim == 2:
        scores, pairs = scores[None], np.asarray(pairs)[None]
    cross = permille if cross is None else cross
    x0, y0, nx, ny, sx, sy = grid
    G = scores.shape[0]
    left = {}
    for o in range(G):
        flat, pr = scores[o].reshape(-1), np.asarray(pairs[o]).reshape(-1)
        bits = flat.view(np.uint32)
        for g in np.flatnonzero(~np.isnan(flat)):
            g = int(g)
            left[(o, g)] = ((int(bits[g]), g, int(pr[g])), sh[int(pr[g])], (x0 + (g % nx) * sx, y0 + (g // nx) * sy))
    out = []
    while len(out) < max_det and left:
        d = min(left, key=lambda e: left[e][0])
        _, D, dt = left.pop(d)
        out.append(d)
        for e in list(left):
            _, S, st = left[e]
            if _suppressed(S, st, D, dt, permille if e[0] == d[0] else cross):
                del left[e]
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def hull_list_nms(entries, max_det, permille, cross=None):
    """The greedy rule on a list: entries are (key, object, Shape, (tx, ty)) with distinct keys; returns the indices of the
    detections in the order found."""
    cross = permille if cross is None else cross
    left = {i: e for i, e in enumerate(entries)}
    out = []
    while len(out) < max_det and left:
        d = min(left, key=lambda i: left[i][0])
        _, do, D, dt = left.pop(d)
        out.append(d)
        for i in list(left):
            _, o, S, st = left[i]
            if _suppressed(S, st, D, dt, permille if o == do else cross):
                del left[i]
    return out
