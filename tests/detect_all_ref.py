"""The numpy definition of "all detections below a score" (include/fdcm.h, "All detections below a score"), the referee of
fdcm_search_exhaustive_detect_all and fdcm_detect_score_bounds, and the arithmetic of the device's early exit (DESIGN.md
section 20).  Not collected: the tests import it.

The call is the greedy rule of nms_ref on the points of the best map whose q is <= max_score (float32 compare; a NaN q has
no candidate anyway): the planes with every other point made NaN / -1, then nms_ref with k = max_detections.

Bound of a template: B = the largest float32 s >= +0 (possibly +inf) with float32(s / den) <= max_score.  Exit rule of the
scoring kernel: with n lines, u = 2^-24 and Bc = B / (1 - 2 n u) rounded upward (exit_bound), a slot whose partial sum C,
the float32 sum of its accumulators at a check, satisfies C > Bc is proved over the bound: its finished sum is > B or NaN."""
import numpy as np

from detect_ref import records
from nms_ref import nms_ref

f32 = np.float32
INF = f32(np.inf)
EXIT_MAX_LINES = 1 << 20


def thresholded(scores, pairs, max_score):
    """The planes of the best map without the points over the threshold: (scores, pairs) with NaN / -1 there."""
    s = np.array(scores, dtype=np.float32)
    p = np.array(pairs, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        over = ~(s <= f32(max_score))
    s[over] = np.nan
    p[over] = -1
    return s, p


def detect_all_ref(scores, pairs, boxes, grid, max_score, max_detections, permille, A=1, cs=None, pivots=None, base=0):
    """(records, footprints) of fdcm_search_exhaustive_detect_all from the planes of the best map."""
    s, p = thresholded(scores, pairs, max_score)
    g, sc, F = nms_ref(s, p, boxes, grid, max_detections, permille)
    return records(g, sc, p, A, cs, pivots, grid, base), F


def denominators(lengths, penalty, tau=1.0):
    """den_t of the best map from fdcm_templates_lengths: max(len, 1e-6), or its float32 power tau (penalty 1); 1 without."""
    lens = np.asarray(lengths, dtype=np.float32)
    if penalty is None:
        return np.ones(lens.shape, dtype=np.float32)
    l = np.maximum(lens, f32(1e-6))
    return l if int(penalty) == 0 else np.power(l, f32(tau)).astype(np.float32)


def quotient_ok(s, den, max_score):
    with np.errstate(all="ignore"):
        return bool(f32(f32(s) / f32(den)) <= f32(max_score))


def score_bound(den, max_score):
    """B by bisection over the bit patterns of the floats >= +0, as the library finds it."""
    bits = lambda b: np.array([b], dtype=np.uint32).view(np.float32)[0]
    top = 0x7F800000
    if quotient_ok(bits(top), den, max_score):
        return INF
    if not quotient_ok(bits(0), den, max_score):
        return f32(0)
    lo, hi = 0, top - 1
    while lo < hi:
        mid = lo + (hi - lo + 1) // 2
        if quotient_ok(bits(mid), den, max_score):
            lo = mid
        else:
            hi = mid - 1
    return bits(lo)


def exit_bound(B, n):
    """Bc: B / (1 - 2 n u) in float64, rounded up to float32 and one float32 further; +inf (no exit) for an infinite B, for
    n > 2^20 and above 1e38."""
    B = f32(B)
    if not B < INF or n > EXIT_MAX_LINES:
        return INF
    f = np.float64(B) / (1.0 - 2.0 * n * 2.0 ** -24)
    c = f32(f)
    if np.float64(c) < f:
        c = np.nextafter(c, INF)
    c = np.nextafter(c, INF)
    return INF if c > f32(1e38) else c


def exit_checks(v):
    """The partial sums C the kernel compares at its checks, in order, for the terms v (n,) float32 summed in capped_ref's
    Eigen order: after each block of 8 while lines remain, C = ((p0[0] + p1[0]) + (p0[1] + p1[1])) + ((p0[2] + p1[2]) +
    (p0[3] + p1[3])) of the two packets; after the trailing packet while lines remain, C = (p0[0] + p0[2]) + (p0[1] + p0[3])
    of p0 = p0 + p1 + packet.  The accumulators start at zero (0 + v == v)."""
    v = np.asarray(v, dtype=np.float32)
    n = len(v)
    a2, a1 = (n // 8) * 8, (n // 4) * 4
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        p0, p1 = np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.float32)
        for b in range(0, a2, 8):
            p0 = p0 + v[b:b + 4]
            p1 = p1 + v[b + 4:b + 8]
            if b + 8 < n:
                out.append(f32(((p0[0] + p1[0]) + (p0[1] + p1[1])) + ((p0[2] + p1[2]) + (p0[3] + p1[3]))))
        p0 = p0 + p1
        if a1 > a2:
            p0 = p0 + v[a2:a2 + 4]
            if a1 < n:
                out.append(f32((p0[0] + p0[2]) + (p0[1] + p0[3])))
    return out
