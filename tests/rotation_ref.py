"""The numpy definition of the exhaustive search over rotations (include/fdcm.h, "Rotations"), the referee of the
device's fdcm_search_exhaustive_rotations.  Not collected: the tests import it.

M_a = [R | m] with R = [[c, -s], [s, c]] and m = p - R p (rotate(lines, R, rot_point), math.h:372-378), every product and
sum in float32, left to right.  key(a, g) = (score bits << 32) | (a N + g) for an admissible point of the (A, ny, nx)
score volume of one template, N = nx ny; NaN is not admissible and has no key.  (a, j, i) is a peak when its key is the
minimum of the keys in its (2 ra + 1) x (2 ry + 1) x (2 rx + 1) window, the angle axis circular with wrap and cut at
0 and A - 1 without."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from peaks_ref import NO_KEY

f32 = np.float32


def rot_matrix(c, s, px=0.0, py=0.0):
    """(2, 3) float32 M_a for one rotation (c, s) and pivot (px, py)."""
    c, s, px, py = f32(c), f32(s), f32(px), f32(py)
    ns = -s
    return np.array([[c, ns, px - (c * px + ns * py)], [s, c, py - (s * px + c * py)]], dtype=np.float32)


def rotate_lines(lines, c, s, px=0.0, py=0.0):
    """(4, N) float32 end points of M_a(lines)."""
    M = rot_matrix(c, s, px, py)
    lines = np.asarray(lines, dtype=np.float32)
    out = np.empty_like(lines)
    for r in (0, 2):
        x, y = lines[r], lines[r + 1]
        out[r] = (M[0, 0] * x + M[0, 1] * y) + M[0, 2]
        out[r + 1] = (M[1, 0] * x + M[1, 1] * y) + M[1, 2]
    return out


def rotated_set(templates, cs, pivots=None):
    """The T * A line sets M_a(t), (t, a) at index t * A + a."""
    out = []
    for t, tm in enumerate(templates):
        px, py = (0.0, 0.0) if pivots is None else pivots[t]
        for c, s in np.asarray(cs, dtype=np.float32).reshape(-1, 2):
            out.append(rotate_lines(np.asarray(tm, dtype=np.float32).reshape(4, -1), c, s, px, py))
    return out


def keys3(vol):
    """(A, ny, nx) uint64 keys of one template's score volume, NO_KEY where it is NaN."""
    vol = np.asarray(vol, dtype=np.float32)
    A, ny, nx = vol.shape
    idx = np.arange(A * ny * nx, dtype=np.uint64).reshape(A, ny, nx)
    k = (vol.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx
    k[np.isnan(vol)] = NO_KEY
    return k


def window_min3(k, rx, ry, ra, wrap):
    """Per point the minimum key of its window: separable, angle first, then rows, then columns."""
    A = k.shape[0]
    m = np.full_like(k, NO_KEY)
    for a in range(A):
        for d in range(-ra, ra + 1):
            b = a + d
            if wrap:
                b %= A
            elif b < 0 or b >= A:
                continue
            m[a] = np.minimum(m[a], k[b])
    p = np.pad(m, ((0, 0), (ry, ry), (rx, rx)), constant_values=NO_KEY)
    rows = sliding_window_view(p, 2 * rx + 1, axis=2).min(axis=-1)
    return sliding_window_view(rows, 2 * ry + 1, axis=1).min(axis=-1)


def peak_mask3(vol, rx, ry, ra, wrap):
    k = keys3(vol)
    return (k != NO_KEY) & (k == window_min3(k, rx, ry, ra, wrap))


def peaks3(vol, k, rx, ry, ra, wrap):
    """The first min(k, count) peaks of one template's volume by key: (a, g, score) arrays."""
    kk = keys3(vol)
    A, ny, nx = kk.shape
    sel = np.sort(kk[(kk != NO_KEY) & (kk == window_min3(kk, rx, ry, ra, wrap))])[:k]
    low = (sel & np.uint64(0xFFFFFFFF)).astype(np.int64)
    s = (sel >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return low // (ny * nx), low % (ny * nx), s


def rotation_peaks_ref(vols, cs, pivots, k, rx, ry, ra, wrap, grid, base=0, skip=()):
    """The records of fdcm_search_exhaustive_rotations for score volumes (T, A, ny, nx) of the grid
    (x0, y0, nx, ny, sx, sy), rotations cs (A, 2) and pivots (T, 2) or None: per template in ascending index (those in
    `skip` left out) its first k peaks, as a structured array of the library's match dtype."""
    from openfdcm_amd import _capi
    x0, y0, nx, ny, sx, sy = grid
    cs = np.asarray(cs, dtype=np.float32).reshape(-1, 2)
    out = []
    for t in range(vols.shape[0]):
        if t in skip:
            continue
        a, g, s = peaks3(vols[t], k, rx, ry, ra, wrap)
        r = np.zeros(len(g), dtype=_capi.MATCH_DTYPE)
        r["tmpl_idx"] = t + base
        r["score"] = s
        px, py = (0.0, 0.0) if pivots is None else pivots[t]
        tr = np.zeros((len(g), 6), dtype=np.float32)
        for q in range(len(g)):
            M = rot_matrix(cs[a[q], 0], cs[a[q], 1], px, py)
            tr[q] = [M[0, 0], M[0, 1], M[0, 2] + f32(x0 + (g[q] % nx) * sx),
                     M[1, 0], M[1, 1], M[1, 2] + f32(y0 + (g[q] // nx) * sy)]
        r["transform"] = tr
        out.append(r)
    return np.concatenate(out) if out else np.zeros(0, dtype=_capi.MATCH_DTYPE)


def brute_peak_mask3(vol, rx, ry, ra, wrap):
    """The definition point by point: for the tests of the referee itself."""
    kk = keys3(vol)
    A, ny, nx = kk.shape
    out = np.zeros(kk.shape, dtype=bool)
    for a in range(A):
        for j in range(ny):
            for i in range(nx):
                if kk[a, j, i] == NO_KEY:
                    continue
                ok = True
                for b in range(A):
                    d = abs(a - b)
                    if wrap:
                        d = min(d, A - d)
                    if d > ra:
                        continue
                    for jj in range(max(0, j - ry), min(ny, j + ry + 1)):
                        for ii in range(max(0, i - rx), min(nx, i + rx + 1)):
                            if (b, jj, ii) != (a, j, i) and kk[b, jj, ii] != NO_KEY and not kk[a, j, i] < kk[b, jj, ii]:
                                ok = False
                out[a, j, i] = ok
    return out
