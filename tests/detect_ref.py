"""The numpy definition of the best map and the detections (include/fdcm.h, "Best map and detections"), the referee of
the device's fdcm_best_map and fdcm_search_exhaustive_detect.  Not collected: the tests import it.

vols is the (T, A, ny, nx) float32 score volume of T templates under A rotations (A = 1: the translations), NaN where a
pair is not admissible.  q(t, a, g) is what fdcm_penalize makes of a record {t, vols[t, a, g]} with the templates'
lengths (penalty None: the score itself).  pairkey(u, g) = (bits of q << 32) | u with u = t A + a; a NaN q has no key, nor
has a template in `skip` (the templates without lines).  best(g) is the pair of the smallest pairkey.  The detections are
the peaks (peaks_ref.py) of the plane of best q."""
import ctypes as C

import numpy as np

from peaks_ref import NO_KEY, brute_peak_mask, peaks
from rotation_ref import rot_matrix

f32 = np.float32


def normalised(vols, lengths, penalty, tau=1.0):
    """q for every entry of vols: fdcm_penalize on the host, a template at a time; penalty None: vols."""
    from openfdcm_amd import _capi
    vols = np.ascontiguousarray(vols, dtype=np.float32)
    if penalty is None:
        return vols.copy()
    lens = np.ascontiguousarray(lengths, dtype=np.float32)
    q = np.empty_like(vols)
    for t in range(vols.shape[0]):
        rec = np.zeros(vols[t].size, dtype=_capi.MATCH_DTYPE)
        rec["tmpl_idx"] = t
        rec["score"] = vols[t].reshape(-1)
        _capi.check(_capi.lib().fdcm_penalize(int(penalty), float(tau), C.c_void_p(rec.ctypes.data), len(rec), _capi.fptr(lens),
                                              len(lens)))
        q[t] = rec["score"].reshape(vols[t].shape)
    return q


def pair_keys(q, skip=()):
    """(T A, ny, nx) uint64 pairkeys of q (T, A, ny, nx), NO_KEY where q is NaN or the template is skipped."""
    T, A, ny, nx = q.shape
    u = np.arange(T * A, dtype=np.uint64).reshape(T * A, 1, 1)
    flat = q.reshape(T * A, ny, nx)
    k = (flat.view(np.uint32).astype(np.uint64) << np.uint64(32)) | u
    k[np.isnan(flat)] = NO_KEY
    for t in skip:
        k[t * A:(t + 1) * A] = NO_KEY
    return k


def best_ref(q, skip=()):
    """(scores (ny, nx) float32 with NaN where no pair has a key, pairs (ny, nx) int32 with -1 there)."""
    T, A, ny, nx = q.shape
    if T * A == 0:
        return np.full((ny, nx), np.nan, dtype=np.float32), np.full((ny, nx), -1, dtype=np.int32)
    m = pair_keys(q, skip).min(axis=0)
    none = m == NO_KEY
    scores = (m >> np.uint64(32)).astype(np.uint32).view(np.float32).copy()
    scores[none] = np.nan
    pairs = (m & np.uint64(0xFFFFFFFF)).astype(np.int64)
    pairs[none] = -1
    return scores, pairs.astype(np.int32)


def brute_best(q, skip=()):
    """best_ref point by point, comparing (q, t, a) as values: for the tests of the referee itself."""
    T, A, ny, nx = q.shape
    scores = np.full((ny, nx), np.nan, dtype=np.float32)
    pairs = np.full((ny, nx), -1, dtype=np.int32)
    for j in range(ny):
        for i in range(nx):
            win = None
            for t in range(T):
                if t in skip:
                    continue
                for a in range(A):
                    v = q[t, a, j, i]
                    if np.isnan(v):
                        continue
                    if win is None or v < win[0]:  # scores are >= +0: the value order is the bit order; ties keep the first
                        win = (v, t * A + a)
            if win is not None:
                scores[j, i], pairs[j, i] = win
    return scores, pairs


def records(g, s, pairs, A, cs, pivots, grid, base=0):
    """Match records of the grid points g (flat indices) with scores s: the pose of the pair pairs[g]."""
    from openfdcm_amd import _capi
    x0, y0, nx, ny, sx, sy = grid
    u = pairs.reshape(-1)[g].astype(np.int64)
    r = np.zeros(len(g), dtype=_capi.MATCH_DTYPE)
    r["tmpl_idx"] = u // A + base
    r["score"] = s
    tr = np.zeros((len(g), 6), dtype=np.float32)
    for n in range(len(g)):
        tx, ty = f32(x0 + (g[n] % nx) * sx), f32(y0 + (g[n] // nx) * sy)
        if cs is None:
            tr[n] = [1, 0, tx, 0, 1, ty]
        else:
            t, a = divmod(int(u[n]), A)
            px, py = (0.0, 0.0) if pivots is None else pivots[t]
            c, s_ = np.asarray(cs, dtype=np.float32).reshape(-1, 2)[a]
            M = rot_matrix(c, s_, px, py)
            tr[n] = [M[0, 0], M[0, 1], M[0, 2] + tx, M[1, 0], M[1, 1], M[1, 2] + ty]
    r["transform"] = tr
    return r


def detect_ref(q, k, rx, ry, grid, cs=None, pivots=None, base=0, skip=()):
    """The records of fdcm_search_exhaustive_detect for normalised scores q (T, A, ny, nx) of the grid
    (x0, y0, nx, ny, sx, sy): the first k peaks of the best plane by key, each with the pose of its best pair.  cs None: the
    translations (A = 1)."""
    scores, pairs = best_ref(q, skip)
    g, s = peaks(scores, k, rx, ry)
    return records(g, s, pairs, q.shape[1], cs, pivots, grid, base)


def brute_detect(q, k, rx, ry, skip=()):
    """(g, score bits, pair) of the detections from the point-by-point forms."""
    scores, pairs = brute_best(q, skip)
    mask = brute_peak_mask(scores, rx, ry)
    g = np.flatnonzero(mask.reshape(-1))
    bits = scores.reshape(-1)[g].view(np.uint32)
    order = np.lexsort((g, bits))[:k]
    return g[order], bits[order], pairs.reshape(-1)[g[order]]
