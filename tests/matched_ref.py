"""The numpy definition of the matched fraction (include/fdcm.h, "Detections by matched fraction"), the referee of
fdcm_search_exhaustive_detect_all_matched, fdcm_matched_fractions and fdcm_templates_matched_totals.  Not collected: the tests
import it.

Line i of a template is matched at a pose when its uncapped cost is <= its cap, one float32 compare: a NaN cost is not
matched, an infinite cost under a cap of +inf is, a cap of 0 is met only by a cost of 0.  ML is the float32 sum of the
matched lines' lengths in line order, from +0; TL the same sum over all lines; frac = ML / TL in float32, 1 when TL == 0.
The gate keeps a grid point when ML of the best map's pair there is >= need = float32(min_matched * TL) of that pair's
template.  The detector's referee is detect_all_ref on the planes `gated` returns."""
import numpy as np

f32 = np.float32


def matched_lengths(cost, caps, lens):
    """ML at every point: cost (n, ...) float32 line costs, caps and lens (n,) -> (...) float32, sequential in line order."""
    cost = np.asarray(cost, dtype=np.float32)
    caps = np.asarray(caps, dtype=np.float32).reshape(-1)
    lens = np.asarray(lens, dtype=np.float32).reshape(-1)
    assert cost.shape[0] == len(caps) == len(lens)
    ml = np.zeros(cost.shape[1:], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(cost.shape[0]):
            ml = np.where(cost[i] <= caps[i], ml + lens[i], ml).astype(np.float32)
    return ml


def total(lens):
    """TL of one template: every line matched."""
    tl = f32(0)
    with np.errstate(over="ignore"):
        for v in np.asarray(lens, dtype=np.float32).reshape(-1):
            tl = f32(tl + v)
    return tl


def totals(lens_per_template):
    return np.array([total(l) for l in lens_per_template], dtype=np.float32)


def need(min_matched, tl):
    """need = float32(min_matched * TL), one float32 product."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (f32(min_matched) * np.asarray(tl, dtype=np.float32)).astype(np.float32)


def fractions(ml, tl):
    """frac = ML / TL, one float32 division; 1 where TL == 0."""
    ml, tl = np.broadcast_arrays(np.asarray(ml, dtype=np.float32), np.asarray(tl, dtype=np.float32))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(tl == 0, f32(1), ml / np.where(tl == 0, f32(1), tl)).astype(np.float32)


def gated(scores, pairs, ml_of_best, need_of_pair):
    """The planes of the best map without the points that fail the gate: (scores, pairs) with NaN / -1 there.  ml_of_best: per
    point ML of the pair the plane holds (anything where there is none); need_of_pair: per pair."""
    s = np.array(scores, dtype=np.float32)
    p = np.array(pairs, dtype=np.int32)
    nd = np.asarray(need_of_pair, dtype=np.float32)[np.where(p >= 0, p, 0)]
    with np.errstate(invalid="ignore"):
        fail = (p >= 0) & ~(np.asarray(ml_of_best, dtype=np.float32) >= nd)
    s[fail] = np.nan
    p[fail] = -1
    return s, p
