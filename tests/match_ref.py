"""The numpy definition of the calls on match lists (include/fdcm.h, "Match lists"), the referee of fdcm_matches_footprints,
fdcm_matches_verify and fdcm_matches_detect.  Not collected: the tests import it.  It works on a volume [k][x][y], the keys
and the scene translation, and never calls the kernels it judges.

A record r is valid when 0 <= t = r.tmpl_idx - base < T.  Its posed lines P(r) are pyoracle.transform of template t by
r.transform (float32, unfused); the bin of a posed line is pyoracle.closest_orientation; r is admissible when every posed
coordinate plus the scene translation lies in (-1, W) x (-1, H); cost_i is |V[bin][int(x1)][int(y1)] - V[bin][int(x2)][int(y2)]|
at the translated, truncated end points; s is pyoracle.eigen_sum of the costs clamped to the caps; ML, TL and frac are
matched_ref's; the footprint is nms_ref.box_of_lines of P(r).  The detect call keeps the records that are valid, have lines,
are admissible, whose q = v / den is not NaN, has a clear sign bit and is <= max_score and whose ML >= need, and runs the
greedy rule on them in Python integers, keyed by (bits of q << 32) | position."""
import numpy as np

import matched_ref
import nms_ref
from helpers import ROOT  # noqa: F401  (puts the repository on sys.path)
from oracle import pyoracle as P

f32 = np.float32
NAN = f32(np.nan)
MATCH_DTYPE = np.dtype([("tmpl_idx", "<i4"), ("score", "<f4"), ("transform", "<f4", (6,))])


def records(tmpl_idx, scores, transforms):
    """A record array from parallel sequences."""
    r = np.zeros(len(tmpl_idx), dtype=MATCH_DTYPE)
    r["tmpl_idx"] = np.asarray(tmpl_idx, dtype=np.int64).astype(np.int32)
    r["score"] = np.asarray(scores, dtype=np.float32)
    r["transform"] = np.asarray(transforms, dtype=np.float32).reshape(len(r), 6)
    return r


def lines_of(templates, t):
    return np.asarray(templates[t], dtype=np.float32).reshape(4, -1)


def posed(templates, rec, base=0):
    """P(r) as a (4, N) float32 array, or None for a record that is not valid."""
    t = int(rec["tmpl_idx"]) - base
    if not 0 <= t < len(templates):
        return None
    with np.errstate(all="ignore"):
        return P.transform(lines_of(templates, t), np.asarray(rec["transform"], dtype=np.float32).reshape(2, 3))


def line_lengths(tm):
    tm = np.asarray(tm, dtype=np.float32).reshape(4, -1)
    with np.errstate(all="ignore"):
        dx, dy = tm[2] - tm[0], tm[3] - tm[1]
        return np.sqrt(dx * dx + dy * dy).astype(np.float32)


def template_lengths(templates):
    """getTemplateLengths: Eigen's sum of the line lengths, per template."""
    return np.array([P.eigen_sum(line_lengths(t)) for t in templates], dtype=np.float32)


def denominators(templates, penalty, tau=1.0):
    """den_t, fdcm_penalize's: 1 without a penalty; max(len, 1e-6) (penalty 0); the C library's powf of that and tau (penalty 1),
    through ctypes as pyoracle takes atanf, so that it is the function the library's host code calls."""
    lens = template_lengths(templates)
    if penalty is None:
        return np.ones(len(lens), dtype=np.float32)
    l = np.maximum(lens, f32(1e-6))
    if int(penalty) == 0:
        return l
    import ctypes
    powf = ctypes.CDLL("libm.so.6").powf
    powf.restype, powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    return np.array([powf(float(v), float(f32(tau))) for v in l], dtype=np.float32)


def flat_caps(templates, caps):
    """One float32 array of caps per template: None (+inf), or one array per template."""
    if caps is None:
        return [np.full(lines_of(templates, t).shape[1], np.inf, dtype=np.float32) for t in range(len(templates))]
    return [np.asarray(c, dtype=np.float32).reshape(-1) for c in caps]


def footprints(templates, recs, base=0, margin=0):
    out = np.zeros((len(recs), 4), dtype=np.int32)
    for j, r in enumerate(recs):
        p = posed(templates, r, base)
        out[j] = nms_ref.EMPTY if p is None else nms_ref.box_of_lines(p, margin)
    return out


def costs_of(vol, keys, t, p):
    """(admissible, costs) of posed lines p on the volume [k][x][y] with scene translation t."""
    W, H = vol.shape[1], vol.shape[2]
    n = p.shape[1]
    with np.errstate(all="ignore"):
        ox, oy = f32(f32(t[0]) + f32(0)), f32(f32(t[1]) + f32(0))
        px, py = (p[[0, 2]] + ox).astype(np.float32), (p[[1, 3]] + oy).astype(np.float32)
        adm = bool(np.all((px > f32(-1)) & (px < f32(W)) & (py > f32(-1)) & (py < f32(H))))   # a NaN fails
    if not adm:
        return False, np.full(n, NAN, dtype=np.float32)
    c = np.zeros(n, dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(n):
            v = vol[P.closest_orientation(keys, p[:, i])]
            c[i] = abs(f32(v[int(px[0, i]), int(py[0, i])] - v[int(px[1, i]), int(py[1, i])]))
    return True, c


def verify(vol, keys, t, templates, recs, base=0, caps=None):
    """(scores (n,), fractions (n,), costs (n, Lmax)) of fdcm_matches_verify, then ML (n,) and admissible (n,)."""
    vol = np.asarray(vol, dtype=np.float32)
    caps = flat_caps(templates, caps)
    lmax = max([lines_of(templates, i).shape[1] for i in range(len(templates))], default=0)
    n = len(recs)
    s, fr, ml = np.full(n, NAN, dtype=np.float32), np.full(n, NAN, dtype=np.float32), np.full(n, NAN, dtype=np.float32)
    costs = np.full((n, lmax), NAN, dtype=np.float32)
    ok = np.zeros(n, dtype=bool)
    for j, r in enumerate(recs):
        p = posed(templates, r, base)
        if p is None:
            continue
        ti = int(r["tmpl_idx"]) - base
        adm, c = costs_of(vol, keys, t, p)
        costs[j, :len(c)] = c
        ok[j] = adm
        if not adm:
            continue
        with np.errstate(all="ignore"):
            s[j] = P.eigen_sum(np.where(c > caps[ti], caps[ti], c).astype(np.float32))
            lens = line_lengths(templates[ti])
            ml[j] = matched_ref.matched_lengths(c, caps[ti], lens) if len(c) else f32(0)
            fr[j] = matched_ref.fractions(ml[j], matched_ref.total(lens))
    return s, fr, costs, ml, ok


def overlaps(a, b, permille):
    """1000 I > permille U for two boxes, in Python integers."""
    a, b = [int(v) for v in a], [int(v) for v in b]
    inter = max(0, min(a[2], b[2]) - max(a[0], b[0]) + 1) * max(0, min(a[3], b[3]) - max(a[1], b[1]) + 1)
    union = (a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - inter
    return 1000 * inter > permille * union


def detect(vol, keys, t, templates, recs, base=0, max_score=np.inf, max_detections=1024, permille=300, margin=0, den=None,
           min_matched=0.0, rescore=False, caps=None, verified=None):
    """(records, indices, boxes, matched) of fdcm_matches_detect.  den: the penalty's denominator per template, or None.
    verified: what verify returned for these records with these caps, when the caller has it already."""
    s, fr, _, ml, adm = verified if verified is not None else verify(vol, keys, t, templates, recs, base, caps)
    F = footprints(templates, recs, base, margin)
    T = len(templates)
    den = np.ones(T, dtype=np.float32) if den is None else np.asarray(den, dtype=np.float32)
    tl = matched_ref.totals([line_lengths(x) for x in templates]) if T else np.zeros(0, dtype=np.float32)
    need = matched_ref.need(min_matched, tl)
    q = np.full(len(recs), NAN, dtype=np.float32)
    left = {}
    for j, r in enumerate(recs):
        ti = int(r["tmpl_idx"]) - base
        if not 0 <= ti < T:
            continue
        with np.errstate(all="ignore"):
            q[j] = f32((s[j] if rescore else r["score"]) / den[ti])
        if lines_of(templates, ti).shape[1] == 0 or not adm[j] or np.isnan(q[j]) or np.signbit(q[j]) or not q[j] <= f32(max_score):
            continue
        if min_matched > 0 and not ml[j] >= need[ti]:
            continue
        left[j] = (int(q[j:j + 1].view(np.uint32)[0]) << 32) | j
    out = []
    cand = np.array(sorted(left, key=left.get), dtype=np.int64)   # S_0 ascending by key; the rule in int64 (areas < 2^53)
    B = F[cand].astype(np.int64).reshape(-1, 4)
    area = (B[:, 2] - B[:, 0] + 1) * (B[:, 3] - B[:, 1] + 1)
    alive = np.ones(len(cand), dtype=bool)
    while alive.any() and len(out) < max_detections:
        d = int(np.argmax(alive))
        out.append(int(cand[d]))
        w = np.maximum(0, np.minimum(B[:, 2], B[d, 2]) - np.maximum(B[:, 0], B[d, 0]) + 1)
        h = np.maximum(0, np.minimum(B[:, 3], B[d, 3]) - np.maximum(B[:, 1], B[d, 1]) + 1)
        inter = w * h
        alive &= ~(1000 * inter > permille * (area + area[d] - inter))
        alive[d] = False
    idx = np.array(out, dtype=np.int32)
    res = np.array(recs[idx], dtype=MATCH_DTYPE) if len(idx) else np.zeros(0, dtype=MATCH_DTYPE)
    res["score"] = q[idx]
    return res, idx, F[idx].reshape(-1, 4).astype(np.int32), fr[idx].astype(np.float32)
