"""The numpy / Python-integer statement of the match lists with objects and hull shapes (include/fdcm.h, "Match lists: objects
and hull shapes"), the referee of fdcm_matches_detect_objects, fdcm_matches_footprint_spans and fdcm_matches_shapes.  Not
collected: the tests import it.  It is the composition of match_ref.verify (s, ML, frac, admissibility), match_ref.posed (P(r)),
hull_ref.Shape (the shape of posed lines) and hull_ref.hull_list_nms (the greedy rule with two limits), with a box-shaped Shape
for BOX sets, and never calls the kernels it judges.

  BoxShape        F(r) as a Shape: every row of the box is full
  rows_by_edges   hull_ref.Shape's rows from the edges of hull_ref.hull instead of all vertex pairs -- the header's remark that the
                  ends of a row of a convex polygon lie on its boundary -- in Python integers; a template of 130 lines at a margin
                  has 1040 vertices, for which rows_by_pairs takes seconds per record.  tests/test_match_objects_definition.py
                  holds it against rows_by_pairs and rows_by_halfplanes.
  Shapes          the Shape of every record of a list at one margin, built once and reused
  candidates      S_0 with its keys
  detect          (records, indices, boxes, matched) of fdcm_matches_detect_objects"""
import numpy as np

import hull_ref
import match_ref as R
import matched_ref
import nms_ref

f32 = np.float32


class BoxShape:
    """The box (x0, y0, x1, y1) as a shape: xl = 0 and xr = x1 - x0 in every row."""

    def __init__(self, box):
        self.box = tuple(int(v) for v in box)
        n = max(0, self.box[3] - self.box[1] + 1)
        self.xl = np.zeros(n, dtype=np.int64)
        self.xr = np.full(n, self.box[2] - self.box[0], dtype=np.int64)
        self.area = int(np.maximum(0, self.xr - self.xl + 1).sum())


def rows_by_edges(verts):
    """{y: (xl, xr)} as hull_ref.rows_by_pairs gives it, from the hull's edges alone."""
    if not verts:
        return {}
    h = hull_ref.hull(verts)
    out = {y: [None, None] for y in range(min(v[1] for v in verts), max(v[1] for v in verts) + 1)}
    for e in range(len(h)):
        p, q = h[e], h[(e + 1) % len(h)]
        if p[1] > q[1]:
            p, q = q, p
        for y in range(p[1], q[1] + 1):
            if p[1] == q[1]:
                lo, hi = min(p[0], q[0]), max(p[0], q[0])
            else:
                dy, num = q[1] - p[1], p[0] * (q[1] - p[1]) + (q[0] - p[0]) * (y - p[1])
                lo, hi = -((-num) // dy), num // dy
            r = out[y]
            r[0] = lo if r[0] is None else min(r[0], lo)
            r[1] = hi if r[1] is None else max(r[1], hi)
    return {y: (r[0], r[1]) for y, r in out.items()}


class Shapes:
    """shape(j): the Shape of record j of `recs` at `margin` -- hull_ref.Shape of P(r_j) for a hull set, BoxShape of F(r_j) for a
    box set -- or None for an invalid record; built on first use and kept."""

    def __init__(self, templates, recs, base=0, margin=0, hull=True, statement=rows_by_edges):
        self.templates, self.recs, self.base, self.margin, self.hull, self.statement = templates, recs, base, margin, hull, statement
        self._made = {}

    def shape(self, j):
        if j not in self._made:
            p = R.posed(self.templates, self.recs[j], self.base)
            if p is None:
                self._made[j] = None
            elif self.hull:
                self._made[j] = hull_ref.Shape(p, self.margin, self.statement)
            else:
                self._made[j] = BoxShape(nms_ref.box_of_lines(p, self.margin))
        return self._made[j]

    def span_table(self, which=None):
        """hull_ref.span_table over the records; which: a boolean mask, the others (and invalid records) with no rows, area 0."""
        sh = []
        for j in range(len(self.recs)):
            s = self.shape(j) if which is None or which[j] else None
            sh.append(s if s is not None else BoxShape((0, 0, -1, -1)))
        return hull_ref.span_table(sh)


def per_object(v, G):
    a = np.asarray(v, dtype=np.float32)
    return np.full(G, a, dtype=np.float32) if a.ndim == 0 else a


def candidates(templates, recs, objects, verified, base=0, max_score=np.inf, min_matched=None, den=None, rescore=False):
    """({position j: key}, q) of S_0; verified: match_ref.verify's tuple for these records."""
    s, fr, _, ml, adm = verified
    T = len(templates)
    objects = np.asarray(objects, dtype=np.int64)
    G = int(objects.max()) + 1 if len(objects) else 1
    ms = per_object(max_score, G)
    mm = None if min_matched is None else per_object(min_matched, G)
    den = np.ones(T, dtype=np.float32) if den is None else np.asarray(den, dtype=np.float32)
    tl = matched_ref.totals([R.line_lengths(x) for x in templates]) if T else np.zeros(0, dtype=np.float32)
    q = np.full(len(recs), R.NAN, dtype=np.float32)
    left = {}
    for j, r in enumerate(recs):
        ti = int(r["tmpl_idx"]) - base
        if not 0 <= ti < T:
            continue
        o = int(objects[ti])
        with np.errstate(all="ignore"):
            q[j] = f32((s[j] if rescore else r["score"]) / den[ti])
        if R.lines_of(templates, ti).shape[1] == 0 or not adm[j] or np.isnan(q[j]) or np.signbit(q[j]) or not q[j] <= f32(ms[o]):
            continue
        if mm is not None and mm[o] > 0:
            with np.errstate(all="ignore"):
                need = f32(f32(mm[o]) * tl[ti])
            if not ml[j] >= need:
                continue
        left[j] = (int(q[j:j + 1].view(np.uint32)[0]) << 32) | j
    return left, q


def detect(templates, recs, objects, verified, shapes, base=0, max_score=np.inf, min_matched=None, max_detections=1024, permille=300,
           cross=None, den=None, rescore=False):
    """(records, indices, boxes, matched) of fdcm_matches_detect_objects.  shapes: a Shapes of these records at the call's
    margin and kind; verified: match_ref.verify's tuple for these records and caps."""
    left, q = candidates(templates, recs, objects, verified, base, max_score, min_matched, den, rescore)
    objects = np.asarray(objects, dtype=np.int64)
    cand = sorted(left, key=left.get)
    entries = [(left[j], int(objects[int(recs[j]["tmpl_idx"]) - base]), shapes.shape(j), (0, 0)) for j in cand]
    kept = hull_ref.hull_list_nms(entries, max_detections, permille, permille if cross is None else cross)
    idx = np.array([cand[i] for i in kept], dtype=np.int32)
    res = np.array(recs[idx], dtype=R.MATCH_DTYPE) if len(idx) else np.zeros(0, dtype=R.MATCH_DTYPE)
    res["score"] = q[idx]
    F = R.footprints(templates, recs[idx], base, shapes.margin) if len(idx) else np.zeros((0, 4), dtype=np.int32)
    return res, idx, F.reshape(-1, 4).astype(np.int32), verified[1][idx].astype(np.float32)
