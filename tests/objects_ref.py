"""The numpy statement of the detector with objects (include/fdcm.h, "Objects"), the referee of fdcm_best_map_objects,
fdcm_search_exhaustive_detect_objects and fdcm_search_exhaustive_detect_windows_objects.  Not collected: the tests import it.

It is built from the referees that are already there.  Templates carry a label objects[t] in [0, G); an entry is a (grid
point, object) pair and keeps the best pair among its object's templates:

  objects_best     plane o is gate_ref.gated_best with every template of another object skipped, at min_matched[o]
  objects_winner   the gate of FDCM_GATE_WINNER: plane o is detect_ref.best_ref of object o's templates without the points whose
                   pair fails matched_ref's gate at min_matched[o]
  objects_nms      the greedy rule over all planes: entries ordered by (bits of q, g, pair); a detection removes the entries
                   of its own object with 1000 I > permille U and those of other objects with 1000 I > cross U
  brute_objects_nms  the same entry by entry in Python integers
  windows_objects_ref  the windows' call: the candidates are window_detect_ref's, object by object with that object's
                   threshold and need and no suppression; the rule with two limits then runs on keys (bits of q, job)"""
import numpy as np

from detect_all_ref import thresholded
from detect_ref import best_ref, records
from gate_ref import gated_best, of_best
from matched_ref import gated, need, totals
from nms_ref import point_boxes
from window_detect_ref import detect_windows_ref

f32 = np.float32


def _skip_for(objects, o, skip):
    return sorted(set(skip) | {t for t, ob in enumerate(objects) if ob != o})


def objects_best(q, ml, objects, G, min_matched, lens, skip=()):
    """(scores, pairs, fractions), each (G, ny, nx): NaN / -1 / NaN where the entry has no candidate.  q, ml: (T, A, ny, nx);
    objects: (T,) labels; min_matched: (G,); lens: per template its lines' lengths; skip: the templates without lines."""
    planes = [gated_best(q, ml, float(min_matched[o]), lens, _skip_for(objects, o, skip)) for o in range(G)]
    return tuple(np.stack([p[c] for p in planes]) for c in range(3))


def objects_winner(q, ml, objects, G, min_matched, lens, skip=()):
    """(scores, pairs) of gate WINNER, each (G, ny, nx): the ungated best pair of the entry, dropped when it fails the gate."""
    T, A = q.shape[:2]
    flat_ml = ml.reshape((T * A,) + ml.shape[2:])
    tl = np.repeat(totals(lens), A)
    out = []
    for o in range(G):
        s0, p0 = best_ref(q, _skip_for(objects, o, skip))
        out.append(gated(s0, p0, of_best(flat_ml, p0), need(float(min_matched[o]), tl)))
    return np.stack([s for s, _ in out]), np.stack([p for _, p in out])


def objects_thresholded(scores, pairs, max_score):
    """The planes without the entries over their object's threshold."""
    out = [thresholded(scores[o], pairs[o], max_score[o]) for o in range(len(scores))]
    return np.stack([s for s, _ in out]), np.stack([p for _, p in out])


def _check_labels(pairs, boxes, objects):
    P = np.asarray(boxes).reshape(-1, 4).shape[0]
    A = P // max(1, len(objects))
    for o in range(len(pairs)):
        u = np.asarray(pairs[o]).reshape(-1)
        u = u[u >= 0]
        assert all(objects[int(v) // A] == o for v in u), "a plane holds a pair of another object"


def objects_nms(scores, pairs, boxes, grid, objects, max_det, permille, cross):
    """The detections as (n, 2) int64 rows (object, flat grid index), in the order found.  scores, pairs: (G, ny, nx) planes
    (NaN / -1: no entry); boxes: (P, 4) per pair; objects: (T,) labels, checked against the planes."""
    scores = np.asarray(scores, dtype=np.float32)
    pairs = np.asarray(pairs, dtype=np.int64)
    G = scores.shape[0]
    N = scores.shape[1] * scores.shape[2]
    _check_labels(pairs, boxes, objects)
    bits = scores.reshape(-1).view(np.uint32).astype(np.int64)
    g = np.tile(np.arange(N, dtype=np.int64), G)
    obj = np.repeat(np.arange(G, dtype=np.int64), N)
    u = pairs.reshape(-1)
    left = ~np.isnan(scores.reshape(-1))
    rank = np.full(G * N, G * N, dtype=np.int64)
    order = np.lexsort((u, g, bits))
    order = order[left[order]]
    rank[order] = np.arange(len(order))
    F = np.concatenate([point_boxes(pairs[o], boxes, grid) for o in range(G)])
    area = (F[:, 2] - F[:, 0] + 1) * (F[:, 3] - F[:, 1] + 1)
    out = []
    while len(out) < max_det and left.any():
        d = int(np.argmin(np.where(left, rank, G * N)))
        out.append((int(obj[d]), int(g[d])))
        w = np.maximum(0, np.minimum(F[:, 2], F[d, 2]) - np.maximum(F[:, 0], F[d, 0]) + 1)
        h = np.maximum(0, np.minimum(F[:, 3], F[d, 3]) - np.maximum(F[:, 1], F[d, 1]) + 1)
        inter = w * h
        union = area + area[d] - inter
        limit = np.where(obj == obj[d], permille, cross)
        left &= ~(1000 * inter > limit * union)
        left[d] = False
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def brute_objects_nms(scores, pairs, boxes, grid, max_det, permille, cross):
    """The rule entry by entry in Python integers: (n, 2) rows (object, flat grid index)."""
    scores = np.asarray(scores, dtype=np.float32)
    x0, y0, nx, ny, sx, sy = grid
    G = scores.shape[0]
    boxes = np.asarray(boxes).reshape(-1, 4)
    left = {}
    for o in range(G):
        flat = scores[o].reshape(-1)
        bits = flat.view(np.uint32)
        pr = np.asarray(pairs[o]).reshape(-1)
        for g in range(nx * ny):
            if np.isnan(flat[g]):
                continue
            b = [int(v) for v in boxes[pr[g]]]
            tx, ty = x0 + (g % nx) * sx, y0 + (g // nx) * sy
            left[(o, g)] = ((int(bits[g]), g, int(pr[g])), (b[0] + tx, b[1] + ty, b[2] + tx, b[3] + ty))
    out = []
    while len(out) < max_det and left:
        d = min(left, key=lambda e: left[e][0])
        D = left.pop(d)[1]
        out.append(d)
        for e in list(left):
            E = left[e][1]
            inter = max(0, min(E[2], D[2]) - max(E[0], D[0]) + 1) * max(0, min(E[3], D[3]) - max(E[1], D[1]) + 1)
            union = (E[2] - E[0] + 1) * (E[3] - E[1] + 1) + (D[2] - D[0] + 1) * (D[3] - D[1] + 1) - inter
            if 1000 * inter > (permille if e[0] == d[0] else cross) * union:
                del left[e]
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def detect_objects_ref(scores, pairs, boxes, grid, objects, max_score, max_det, permille, cross, A=1, cs=None, pivots=None,
                       fractions=None, base=0):
    """(records, footprints (n, 4) int32, fractions (n,) float32 or None, entries (n, 2)) of
    fdcm_search_exhaustive_detect_objects from the planes of the object best map (gated as the call's gate says)."""
    from openfdcm_amd import _capi
    s, p = objects_thresholded(scores, pairs, max_score)
    ent = objects_nms(s, p, boxes, grid, objects, max_det, permille, cross)
    rec = np.zeros(len(ent), dtype=_capi.MATCH_DTYPE)
    F = np.zeros((len(ent), 4), dtype=np.int32)
    fr = np.zeros(len(ent), dtype=np.float32)
    for l, (o, g) in enumerate(ent):
        rec[l] = records(np.array([g]), s[o].reshape(-1)[[g]], p[o], A, cs, pivots, grid, base)[0]
        F[l] = point_boxes(p[o], boxes, grid)[g]
        if fractions is not None:
            fr[l] = np.asarray(fractions[o]).reshape(-1)[g]
    return rec, F, (fr if fractions is not None else None), ent


def windows_objects_ref(vols, master, jobs, cs, pivots, sx, sy, den, boxes, objects, max_score, min_matched, max_det, permille, cross,
                        costs, caps, lens):
    """(records, boxes, fractions, jobs) of fdcm_search_exhaustive_detect_windows_objects at FDCM_GATE_WINNER (for
    FDCM_GATE_ALL hand in gate_ref.gated_volumes per object and min_matched of zeros: see the caller).  vols may be one list
    for all objects or a list per object."""
    jobs = np.asarray(jobs).reshape(-1, 7)
    G = len(max_score)
    per_object = isinstance(vols, dict)
    cand = []  # (key, job, object, record, box, fraction)
    for o in range(G):
        idx = np.flatnonzero(np.asarray(objects)[jobs[:, 0]] == o)
        if len(idx) == 0:
            continue
        rec, F, fr, ji, _ = detect_windows_ref(vols[o] if per_object else vols, master, jobs[idx], cs, pivots, sx, sy, den, boxes,
                                               max_score[o], len(idx) + 1, 1000, float(min_matched[o]), costs, caps, lens)
        for l in range(len(rec)):
            j = int(idx[ji[l]])
            cand.append(((int(rec["score"][l:l + 1].view(np.uint32)[0]) << 32) | j, j, o, rec[l], [int(v) for v in F[l]], fr[l]))
    cand.sort(key=lambda c: c[0])
    out = []
    while len(out) < max_det and cand:
        D = cand.pop(0)
        out.append(D)
        keep = []
        for c in cand:
            E, B = c[4], D[4]
            inter = max(0, min(E[2], B[2]) - max(E[0], B[0]) + 1) * max(0, min(E[3], B[3]) - max(E[1], B[1]) + 1)
            union = (E[2] - E[0] + 1) * (E[3] - E[1] + 1) + (B[2] - B[0] + 1) * (B[3] - B[1] + 1) - inter
            if not 1000 * inter > (permille if c[2] == D[2] else cross) * union:
                keep.append(c)
        cand = keep
    from openfdcm_amd import _capi
    rec = np.zeros(len(out), dtype=_capi.MATCH_DTYPE)
    for l, c in enumerate(out):
        rec[l] = c[3]
    return (rec, np.array([c[4] for c in out], dtype=np.int32).reshape(-1, 4), np.array([c[5] for c in out], dtype=np.float32),
            np.array([c[1] for c in out], dtype=np.int32))
