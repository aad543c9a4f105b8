"""The numpy statement of the gate inside the minimum (include/fdcm.h, "Gate inside the minimum"), the referee of
fdcm_best_map_gated, fdcm_search_exhaustive_detect_all_gated and fdcm_search_exhaustive_detect_windows_gated at
FDCM_GATE_ALL.  Not collected: the tests import it.

It is built from the referees that are already there and never calls a gated or a capped path.  The inputs are the uncapped
cost maps of the lines (capped_ref.line_cost_maps: the score maps of one-line templates), from which come the capped scores
(capped_ref.capped_volumes), q (detect_ref.normalised) and ML of every pair at every point (matched_ref.matched_lengths).

  gate ALL, dense     q of a pair at a point becomes NaN where ML < need of its template; detect_ref.best_ref on that q gives
                      the planes (a NaN q has no key), detect_all_ref.detect_all_ref the records
  gate ALL, windows   the score volumes with the failing poses made NaN go through window_detect_ref.detect_windows_ref with
                      min_matched = 0: the winner is the smallest key among the poses that pass
  gate WINNER         matched_ref.gated on the planes of the unrestricted best map, as before"""
import numpy as np

from detect_ref import best_ref
from matched_ref import fractions, matched_lengths, need, totals

f32 = np.float32


def pair_matched_lengths(cost, offsets, caps, lens):
    """ML of every pair at every point: cost (L, A, ...) uncapped line costs, template t's lines offsets[t] .. offsets[t + 1],
    caps[t] and lens[t] its lines' caps and lengths -> (T, A, ...) float32."""
    T = len(offsets) - 1
    out = np.zeros((T,) + cost.shape[1:], dtype=np.float32)
    for t in range(T):
        out[t] = matched_lengths(cost[offsets[t]:offsets[t + 1]], caps[t], lens[t])
    return out


def passes(ml, min_matched, tl):
    """(T, A, ...) bool: ML >= need_t, need_t = float32(min_matched * TL_t); one float32 compare, false for a NaN."""
    nd = need(min_matched, tl).reshape((-1,) + (1,) * (ml.ndim - 1))
    with np.errstate(invalid="ignore"):
        return np.asarray(ml, dtype=np.float32) >= nd


def gated_q(q, ml, min_matched, tl):
    """q (T, A, ...) with NaN where the pair fails the gate there: such a pair is no candidate of the point."""
    out = np.array(q, dtype=np.float32)
    out[~passes(ml, min_matched, tl)] = np.nan
    return out


def of_best(maps, pairs):
    """Per grid point the value of maps (P, ny, nx) for the pair the plane holds there (pair 0's where there is none)."""
    p = np.asarray(pairs).reshape(-1)
    flat = np.asarray(maps).reshape(maps.shape[0], -1)
    return flat[np.where(p >= 0, p, 0), np.arange(p.size)].reshape(np.asarray(pairs).shape)


def gated_best(q, ml, min_matched, lens, skip=()):
    """The planes of the gated best map: (scores, pairs, fractions), NaN / -1 / NaN where the point has no candidate.
    q, ml: (T, A, ny, nx); lens: per template its lines' lengths; skip: the templates without lines."""
    tl = totals(lens)
    T, A = q.shape[:2]
    scores, pairs = best_ref(gated_q(q, ml, min_matched, tl), skip)
    frac = fractions(ml, tl.reshape(-1, 1, 1, 1)).reshape((T * A,) + q.shape[2:])
    fr = of_best(frac, pairs).astype(np.float32)
    fr[pairs < 0] = np.nan
    return scores, pairs, fr


def gated_volumes(vols, ml, min_matched, lens):
    """Windows: per template its (A, NY, NX) score volume with the failing poses made NaN (None stays None)."""
    tl = totals(lens)
    out = []
    for t, v in enumerate(vols):
        if v is None:
            out.append(None)
            continue
        g = np.array(v, dtype=np.float32)
        g[~passes(ml[t][None], min_matched, tl[t:t + 1])[0]] = np.nan
        out.append(g)
    return out
