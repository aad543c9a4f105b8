"""The numpy definition of the exhaustive search's peaks (include/fdcm.h, "Peaks"), the referee of the device's
fdcm_search_exhaustive_peaks.  Not collected: the tests import it.

key(p) = (score bits << 32) | g for an admissible point p of a (ny, nx) score map, g = j nx + i; NaN is not admissible and
has no key.  p is a peak when key(p) is the minimum of the keys in its (2 ry + 1) x (2 rx + 1) window, neighbours outside
the map or without a key ignored."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def keys(plane):
    """(ny, nx) uint64 keys of one float32 score map, NO_KEY where it is NaN."""
    plane = np.asarray(plane, dtype=np.float32)
    ny, nx = plane.shape
    g = np.arange(ny * nx, dtype=np.uint64).reshape(ny, nx)
    k = (plane.view(np.uint32).astype(np.uint64) << np.uint64(32)) | g
    k[np.isnan(plane)] = NO_KEY
    return k


def window_min(k, rx, ry):
    """Per point the minimum key of its window: separable, rows then columns (min is associative), NO_KEY padding."""
    p = np.pad(k, ((ry, ry), (rx, rx)), constant_values=NO_KEY)
    rows = sliding_window_view(p, 2 * rx + 1, axis=1).min(axis=-1)  # (ny + 2 ry, nx)
    return sliding_window_view(rows, 2 * ry + 1, axis=0).min(axis=-1)  # (ny, nx)


def peak_mask(plane, rx, ry):
    """(ny, nx) bool: the peaks of one score map."""
    k = keys(plane)
    return (k != NO_KEY) & (k == window_min(k, rx, ry))


def peaks(plane, k, rx, ry):
    """The first min(k, count) peaks of one score map by key: (g, score) arrays."""
    kk = keys(plane)
    sel = np.sort(kk[(kk != NO_KEY) & (kk == window_min(kk, rx, ry))])[:k]
    g = (sel & np.uint64(0xFFFFFFFF)).astype(np.int64)
    s = (sel >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return g, s


def peaks_ref(maps, k, rx, ry, grid, base=0, skip=()):
    """The records of fdcm_search_exhaustive_peaks for score maps (T, ny, nx) of the grid (x0, y0, nx, ny, sx, sy):
    per template in ascending index (those in `skip`, the templates without lines, left out) its first k peaks, as a
    structured array of the library's match dtype."""
    from openfdcm_amd import _capi
    x0, y0, nx, ny, sx, sy = grid
    out = []
    for t in range(maps.shape[0]):
        if t in skip:
            continue
        g, s = peaks(maps[t], k, rx, ry)
        r = np.zeros(len(g), dtype=_capi.MATCH_DTYPE)
        r["tmpl_idx"] = t + base
        r["score"] = s
        tr = np.zeros((len(g), 6), dtype=np.float32)
        tr[:, 0] = tr[:, 4] = 1
        tr[:, 2] = x0 + (g % nx) * sx
        tr[:, 5] = y0 + (g // nx) * sy
        r["transform"] = tr
        out.append(r)
    return np.concatenate(out) if out else np.zeros(0, dtype=_capi.MATCH_DTYPE)


def brute_peak_mask(plane, rx, ry):
    """The definition point by point, O(n r^2): for the tests of the referee itself."""
    kk = keys(plane)
    ny, nx = kk.shape
    out = np.zeros((ny, nx), dtype=bool)
    for j in range(ny):
        for i in range(nx):
            if kk[j, i] == NO_KEY:
                continue
            ok = True
            for jj in range(max(0, j - ry), min(ny, j + ry + 1)):
                for ii in range(max(0, i - rx), min(nx, i + rx + 1)):
                    if (jj, ii) != (j, i) and kk[jj, ii] != NO_KEY and not kk[j, i] < kk[jj, ii]:
                        ok = False
            out[j, i] = ok
    return out
