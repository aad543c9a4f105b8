"""The definition of scene coverage and selection of match records (include/fdcm.h, "Match lists: scene coverage and
selection") in numpy and plain Python integers, the referee of fdcm_matches_coverage and fdcm_matches_select.  Not collected:
the tests import it.  It needs no device and nothing here comes from the kernel.

It takes the keys, the scene translation T, the map size (W, H), the labels, the templates and the records.  Posing, bins,
admissibility and footprints are match_ref's (pyoracle.transform, float32 and unfused; pyoracle.closest_orientation on the
host libm's atanf; every posed coordinate plus T in (-1, W) x (-1, H); nms_ref.box_of_lines of the posed lines).  The segment of
a line joins trunc(fl(p + fl(T + 0))) of its two posed end points, moved by -(bx, by) (coverage_ref.end_pixels at the
translation (0, 0), coverage_ref.frame); the window is the footprint at the margin cut to the image; the test is
coverage_ref.near_segment_many and bin_distance; the rule is select_ref.rule."""
import numpy as np

from helpers import ROOT  # noqa: F401  (puts the repository on sys.path)
import coverage_ref as CR
import match_ref as MR
import select_ref as SR
from oracle import pyoracle as P

f32 = np.float32


def segments(keys, T, W, H, templates, rec, base=0):
    """None for a record that is not valid; else (admissible, (4, N) int64 map pixels ax, ay, bx, by, (N,) int64 bins, the
    (4, N) float32 posed lines)."""
    p = MR.posed(templates, rec, base)
    if p is None:
        return None
    ok, ends = CR.end_pixels(p, T, W, H, 0, 0)
    if not ok:
        return False, ends, np.zeros(0, dtype=np.int64), p
    with np.errstate(all="ignore"):
        bins = np.array([P.closest_orientation(keys, p[:, i]) for i in range(p.shape[1])], dtype=np.int64)
    return True, ends, bins, p


def window(templates, rec, base, margin, width, height):
    """x0, y0, x1, y1 of the record's window, cut to the image (x0 > x1 or y0 > y1: empty)."""
    x0, y0, x1, y1 = (int(v) for v in MR.footprints(templates, [rec], base, margin)[0])
    return max(0, x0), max(0, y0), min(width - 1, x1), min(height - 1, y1)


def coverage(labels, keys, T, W, H, templates, recs, base=0, radius=2, bin_tolerance=1, margin=None):
    """(counts (n, 2) int32, residual (height, width) uint8, masks): masks[j] is the (height, width) bool image of the pixels
    record j explains, None for a record that is invalid or not admissible."""
    labels = np.asarray(labels)
    assert labels.ndim == 2 and labels.dtype == np.uint8
    height, width = labels.shape
    keys = np.asarray(keys, dtype=np.float32)
    m = len(keys)
    margin = radius if margin is None else margin
    assert 0 <= radius <= 32 and 0 <= bin_tolerance <= m // 2 and 0 <= margin <= 4096
    bx, by = CR.frame(T, W, H, width, height)
    counts = np.zeros((len(recs), 2), dtype=np.int32)
    residual = labels.copy()
    masks = []
    for j, r in enumerate(recs):
        s = segments(keys, T, W, H, templates, r, base)
        if s is None or not s[0]:
            counts[j] = (-1, -1)
            masks.append(None)
            continue
        _, ends, bins, _ = s
        mask = np.zeros(labels.shape, dtype=bool)
        masks.append(mask)
        x0, y0, x1, y1 = window(templates, r, base, margin, width, height)
        if x0 > x1 or y0 > y1:
            continue
        ys, xs = np.nonzero(labels[y0:y1 + 1, x0:x1 + 1] < m)
        ys, xs = ys + y0, xs + x0
        labs = labels[ys, xs].astype(np.int64)
        hit = np.zeros(len(xs), dtype=bool)
        for i in range(0, ends.shape[1], 64):
            e, b = ends[:, i:i + 64], bins[i:i + 64]
            near = CR.near_segment_many(xs[:, None], ys[:, None], e[0] - bx, e[1] - by, e[2] - bx, e[3] - by, radius)
            hit |= ((CR.bin_distance(labs[:, None], b, m) <= bin_tolerance) & near).any(axis=1)
        counts[j] = (len(xs), int(hit.sum()))
        mask[ys[hit], xs[hit]] = True
        residual[mask] = 255
    return counts, residual, masks


def select(labels, keys, T, W, H, templates, recs, base=0, radius=2, bin_tolerance=1, margin=None, **kw):
    """(selected (k,) int32, counts (k, 3) int32, residual) of fdcm_matches_select: select_ref.rule on this coverage."""
    counts, _, masks = coverage(labels, keys, T, W, H, templates, recs, base, radius, bin_tolerance, margin)
    return SR.rule(labels, counts, masks, **kw)


def translation_records(poses, scores=None):
    """The records {1, 0, x, 0, 1, y} of poses (n, 4) rows (tmpl, 0, x, y)."""
    poses = np.asarray(poses, dtype=np.int64).reshape(-1, 4)
    tf = np.zeros((len(poses), 6), dtype=np.float32)
    tf[:, 0] = tf[:, 4] = 1
    tf[:, 2], tf[:, 5] = poses[:, 2], poses[:, 3]
    return MR.records(poses[:, 0], np.zeros(len(poses)) if scores is None else scores, tf)
