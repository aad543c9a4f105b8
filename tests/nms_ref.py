"""The numpy definition of the detections suppressed by footprint overlap (include/fdcm.h, "Detections suppressed by
footprint overlap"), the referee of fdcm_search_exhaustive_detect_nms and fdcm_templates_footprints.  Not collected: the
tests import it.

Footprint of a pair u = (t, a): over the end points of the lines of M_a(t) (rotation_ref.rot_matrix's float32 rule; without
a table the lines as they are) x0 = floor(min x) - margin, x1 = floor(max x) + margin, y0 and y1 likewise, in exact
integers, clamped to [-2^25, 2^25]; (0, 0, -1, -1) for a template without lines or with a NaN end point.  The footprint of
grid point g is F(g) = box(best(g)) + (x0 + i sx, y0 + j sy), a rectangle of pixels with both ends included.  h suppresses g
when 1000 I > permille U with I the area of F(g) n F(h) and U = A(g) + A(h) - I.  Greedy rule: the point of the smallest
key (peaks_ref.keys) among those left is a detection; it and the points it suppresses leave; at most k times."""
import numpy as np

from detect_ref import records
from peaks_ref import NO_KEY, keys
from rotation_ref import rotate_lines

LIM = 1 << 25
EMPTY = (0, 0, -1, -1)


def box_of_lines(lines, margin=0):
    """(4,) int32 x0, y0, x1, y1 of one (4, N) line array."""
    lines = np.asarray(lines, dtype=np.float32).reshape(4, -1)
    if lines.shape[1] == 0 or np.isnan(lines).any():
        return np.array(EMPTY, dtype=np.int32)
    xs, ys = np.concatenate([lines[0], lines[2]]), np.concatenate([lines[1], lines[3]])

    def at(v, d):  # floor(v) + d as an exact integer (an infinite v: far outside the clamp), clamped
        f = int(np.clip(np.floor(np.float64(v)), -2.0 ** 40, 2.0 ** 40))
        return min(max(f + d, -LIM), LIM)
    return np.array([at(xs.min(), -margin), at(ys.min(), -margin), at(xs.max(), margin), at(ys.max(), margin)], dtype=np.int32)


def footprints(templates, cs=None, pivots=None, margin=0):
    """(T, A, 4) int32 boxes of every (template, rotation); cs None: A = 1, the lines as they are."""
    A = 1 if cs is None else len(np.asarray(cs, dtype=np.float32).reshape(-1, 2))
    out = np.zeros((len(templates), A, 4), dtype=np.int32)
    for t, tm in enumerate(templates):
        tm = np.asarray(tm, dtype=np.float32).reshape(4, -1)
        if cs is None:
            out[t, 0] = box_of_lines(tm, margin)
            continue
        px, py = (0.0, 0.0) if pivots is None else pivots[t]
        for a, (c, s) in enumerate(np.asarray(cs, dtype=np.float32).reshape(-1, 2)):
            out[t, a] = box_of_lines(rotate_lines(tm, c, s, px, py), margin)
    return out


def point_boxes(pairs, boxes, grid):
    """(ny nx, 4) int64 F(g) of every grid point (rows of points without a candidate are meaningless)."""
    x0, y0, nx, ny, sx, sy = grid
    g = np.arange(nx * ny, dtype=np.int64)
    t = np.stack([x0 + (g % nx) * sx, y0 + (g // nx) * sy], axis=1)
    u = np.asarray(pairs, dtype=np.int64).reshape(-1)
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)[np.where(u >= 0, u, 0)]
    return b + np.concatenate([t, t], axis=1)


def nms_ref(scores, pairs, boxes, grid, k, permille):
    """(g, score, F) of the detections: flat grid indices in the order found, float32 scores, (n, 4) int32 footprints.
    scores, pairs: the (ny, nx) planes of the best map (NaN / -1: no candidate); boxes: (P, 4) per pair."""
    kk = keys(scores).reshape(-1)
    F = point_boxes(pairs, boxes, grid)
    area = (F[:, 2] - F[:, 0] + 1) * (F[:, 3] - F[:, 1] + 1)
    left = kk != NO_KEY
    out = []
    while len(out) < k and left.any():
        d = int(np.argmin(np.where(left, kk, NO_KEY)))  # keys are distinct
        out.append(d)
        w = np.maximum(0, np.minimum(F[:, 2], F[d, 2]) - np.maximum(F[:, 0], F[d, 0]) + 1)
        h = np.maximum(0, np.minimum(F[:, 3], F[d, 3]) - np.maximum(F[:, 1], F[d, 1]) + 1)
        inter = w * h
        union = area + area[d] - inter
        left &= ~(1000 * inter > permille * union)
        left[d] = False
    g = np.array(out, dtype=np.int64)
    return g, np.asarray(scores, dtype=np.float32).reshape(-1)[g], F[g].astype(np.int32)


def brute_nms(scores, pairs, boxes, grid, k, permille):
    """The rule point by point in Python integers: the flat grid indices of the detections."""
    scores = np.asarray(scores, dtype=np.float32)
    x0, y0, nx, ny, sx, sy = grid
    bits = scores.reshape(-1).view(np.uint32)
    pairs = np.asarray(pairs).reshape(-1)
    left = {}
    for g in range(nx * ny):
        if np.isnan(scores.reshape(-1)[g]):
            continue
        b = [int(v) for v in np.asarray(boxes).reshape(-1, 4)[pairs[g]]]
        tx, ty = x0 + (g % nx) * sx, y0 + (g // nx) * sy
        left[g] = ((int(bits[g]) << 32) | g, (b[0] + tx, b[1] + ty, b[2] + tx, b[3] + ty))
    out = []
    while len(out) < k and left:
        d = min(left, key=lambda g: left[g][0])
        D = left.pop(d)[1]
        out.append(d)
        for g in list(left):
            G = left[g][1]
            inter = max(0, min(G[2], D[2]) - max(G[0], D[0]) + 1) * max(0, min(G[3], D[3]) - max(G[1], D[1]) + 1)
            union = (G[2] - G[0] + 1) * (G[3] - G[1] + 1) + (D[2] - D[0] + 1) * (D[3] - D[1] + 1) - inter
            if 1000 * inter > permille * union:
                del left[g]
    return np.array(out, dtype=np.int64)


def detect_nms_ref(scores, pairs, boxes, grid, k, permille, A=1, cs=None, pivots=None, base=0):
    """(records, footprints) of fdcm_search_exhaustive_detect_nms from the planes of the best map."""
    g, s, F = nms_ref(scores, pairs, boxes, grid, k, permille)
    return records(g, s, pairs, A, cs, pivots, grid, base), F
