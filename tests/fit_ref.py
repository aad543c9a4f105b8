"""The definition of the pose fit of match records (include/fdcm.h, "Match lists: pose fit") in plain Python integers and
np.float64 scalars, the referee of fdcm_matches_fit.  Not collected: the tests import it.  It needs no device and nothing
here comes from the kernel.

Posing, bins, admissibility, segments and the window are match_coverage_ref's.  The choice of a line for a pixel and the six
moments are Python integers; the normal equations, the solve and the fold are one np.float64 operation per step of the
section, in its order (numpy scalars are IEEE and never fused)."""
import numpy as np

from helpers import ROOT  # noqa: F401  (puts the repository on sys.path)
import coverage_ref as CR
import match_coverage_ref as MC
import match_ref as MR

f32, f64 = np.float32, np.float64
NAN32 = f32(np.nan)


def fit_line(px, py, lab, ends, bins, m, radius, tol):
    """The line the edge pixel (px, py) with label lab is assigned to, or -1, and (wx, wy) = P - A of that line.  ends: (4, N)
    label-frame end pixels."""
    best, r2 = None, radius * radius
    for i in range(ends.shape[1]):
        if int(CR.bin_distance(lab, int(bins[i]), m)) > tol:
            continue
        ax, ay, bx, by = (int(v) for v in ends[:, i])
        dx, dy, wx, wy = bx - ax, by - ay, px - ax, py - ay
        dot, len2 = wx * dx + wy * dy, dx * dx + dy * dy
        if len2 <= 0 or not 0 < dot < len2:
            continue
        cross = wx * dy - wy * dx
        if cross * cross > r2 * len2:
            continue
        if best is None or cross * cross * best[2] < best[1] * len2:   # strict: ties stay with the lowest i
            best = (i, cross * cross, len2, wx, wy)
    return (-1, 0, 0) if best is None else (best[0], best[3], best[4])


def moments_plain(labels, m, ends, bins, window, radius, tol):
    """(N, 6) Python-integer sums S1, Sx, Sy, Sxx, Sxy, Syy per line over the fit pixels of the window (x0, y0, x1, y1): the
    definition as loops over pixels and lines."""
    S = [[0] * 6 for _ in range(ends.shape[1])]
    x0, y0, x1, y1 = window
    if x0 > x1 or y0 > y1:
        return S
    ys, xs = np.nonzero(labels[y0:y1 + 1, x0:x1 + 1] < m)
    for y, x in zip(ys + y0, xs + x0):
        i, wx, wy = fit_line(int(x), int(y), int(labels[y, x]), ends, bins, m, radius, tol)
        if i >= 0:
            for k, v in enumerate((1, wx, wy, wx * wx, wx * wy, wy * wy)):
                S[i][k] += v
    return S


def moments(labels, m, ends, bins, window, radius, tol):
    """moments_plain with the pixels of the window as int64 arrays and a loop over the lines, for the larger cases.  Every
    coordinate is below 2^13 in magnitude here (asserted), so cross^2 len2 stays below 2^62: int64 is exact."""
    n_lines = ends.shape[1]
    S = [[0] * 6 for _ in range(n_lines)]
    x0, y0, x1, y1 = window
    if x0 > x1 or y0 > y1 or n_lines == 0:
        return S
    ys, xs = np.nonzero(labels[y0:y1 + 1, x0:x1 + 1] < m)
    ys, xs = (ys + y0).astype(np.int64), (xs + x0).astype(np.int64)
    labs = labels[ys, xs].astype(np.int64)
    assert np.abs(ends).max() < 1 << 13 and max(labels.shape) < 1 << 13
    bi = np.full(len(xs), -1, dtype=np.int64)
    bc2, bl2 = np.zeros(len(xs), dtype=np.int64), np.ones(len(xs), dtype=np.int64)
    bwx, bwy = np.zeros(len(xs), dtype=np.int64), np.zeros(len(xs), dtype=np.int64)
    r2 = radius * radius
    for i in range(n_lines):
        ax, ay, bx, by = (int(v) for v in ends[:, i])
        dx, dy = bx - ax, by - ay
        len2 = dx * dx + dy * dy
        if len2 == 0:
            continue
        wx, wy = xs - ax, ys - ay
        dot, c2 = wx * dx + wy * dy, (wx * dy - wy * dx) ** 2
        ok = (CR.bin_distance(labs, int(bins[i]), m) <= tol) & (dot > 0) & (dot < len2) & (c2 <= r2 * len2)
        ok &= (bi < 0) | (c2 * bl2 < bc2 * len2)
        bi[ok], bc2[ok], bl2[ok], bwx[ok], bwy[ok] = i, c2[ok], len2, wx[ok], wy[ok]
    for i in np.unique(bi[bi >= 0]):
        wx, wy = bwx[bi == i], bwy[bi == i]
        S[i] = [int(v) for v in (len(wx), wx.sum(), wy.sum(), (wx * wx).sum(), (wx * wy).sum(), (wy * wy).sum())]
    return S


def S_of(p, q, S):
    """S(p, q), left to right."""
    return (p[0] * q[0] * S[0] + (p[0] * q[1] + p[1] * q[0]) * S[1] + (p[0] * q[2] + p[2] * q[0]) * S[2] + p[1] * q[1] * S[3]
            + (p[1] * q[2] + p[2] * q[1]) * S[4] + p[2] * q[2] * S[5])


def float_ends(posed, T, bx, by):
    """pa, pb per line as (4, N) float64: the float32 sums before the truncation, minus the integer border."""
    ox, oy = f32(f32(T[0]) + f32(0)), f32(f32(T[1]) + f32(0))
    q = np.stack([posed[0] + ox, posed[1] + oy, posed[2] + ox, posed[3] + oy]).astype(np.float32)
    return q.astype(np.float64) - np.array([[bx], [by], [bx], [by]], dtype=np.float64)


def normal_equations(S, ends, pf):
    """(N 3x3, v 3, See, n, pivot) from the moments, the label-frame end pixels and the float end points."""
    z = f64(0)
    N = [[z, z, z], [z, z, z], [z, z, z]]
    v, See, n = [z, z, z], z, 0
    if ends.shape[1] == 0:
        return N, v, See, n, (z, z)
    xs, ys = [int(a) for a in ends[[0, 2]].ravel()], [int(a) for a in ends[[1, 3]].ravel()]
    cx, cy = f64((min(xs) + max(xs)) >> 1), f64((min(ys) + max(ys)) >> 1)
    for i in range(ends.shape[1]):
        if S[i][0] == 0:
            continue
        pax, pay, pbx, pby = (f64(a) for a in pf[:, i])
        tx, ty = pbx - pax, pby - pay
        L = np.sqrt(tx * tx + ty * ty)
        if L == 0:
            continue
        nx, ny = ty / L, -tx / L
        ox, oy = f64(int(ends[0, i])), f64(int(ends[1, i]))
        e0 = nx * (ox - pax) + ny * (oy - pay)
        g0 = ny * (ox - cx) - nx * (oy - cy)
        f = [(nx, z, z), (ny, z, z), (g0, ny, -nx)]
        e = (e0, nx, ny)
        Sf = [f64(a) for a in S[i]]
        for r in range(3):
            for s in range(r, 3):
                N[r][s] = N[r][s] + S_of(f[r], f[s], Sf)
            v[r] = v[r] + S_of(f[r], e, Sf)
        See = See + S_of(e, e, Sf)
        n += S[i][0]
    return N, v, See, n, (cx, cy)


def solve_step(N, v, par):
    """(status, x0, x1, x2): 0 with the step, or 2 / 3."""
    mu = f64(par["damping"])
    tr = N[0][0] + N[1][1]
    N00, N11, N22 = N[0][0] + mu * tr, N[1][1] + mu * tr, N[2][2] + mu * N[2][2]
    N01, N02, N12 = N[0][1], N[0][2], N[1][2]
    d0 = N00; l10 = N01 / d0; l20 = N02 / d0
    d1 = N11 - l10 * N01; m21 = N12 - l20 * N01; l21 = m21 / d1
    d2 = N22 - l20 * N02 - l21 * m21
    if not (d0 > 0 and d1 > 0 and d2 > 0):
        return 2, None, None, None
    y0 = v[0]; y1 = v[1] - l10 * y0; y2 = v[2] - l20 * y0 - l21 * y1
    x2 = y2 / d2; x1 = y1 / d1 - l21 * x2; x0 = y0 / d0 - l10 * x1 - l20 * x2
    if not (np.isfinite(x0) and np.isfinite(x1) and np.isfinite(x2)):
        return 2, None, None, None
    if abs(x0) > f64(par["max_shift"]) or abs(x1) > f64(par["max_shift"]) or abs(x2) > f64(par["max_angle"]):
        return 3, None, None, None
    return 0, x0, x1, x2


def fold(M, x0, x1, x2, c):
    """The stepped float32 transform."""
    h = x2 / f64(2); q = h * h
    cc, ss = (f64(1) - q) / (f64(1) + q), (h + h) / (f64(1) + q)
    m0, m1, m2, m3, m4, m5 = (f64(a) for a in M)
    cx, cy = c
    return np.array([cc * m0 - ss * m3, cc * m1 - ss * m4, ((cc * (m2 - cx) - ss * (m5 - cy)) + cx) + x0,
                     ss * m0 + cc * m3, ss * m1 + cc * m4, ((ss * (m2 - cx) + cc * (m5 - cy)) + cy) + x1], dtype=np.float64).astype(np.float32)


def rms_of(See, n):
    return f32(np.sqrt((See if See > 0 else f64(0)) / f64(n))) if n > 0 else NAN32


def pass_of(labels, keys, T, W, H, templates, rec, base, radius, tol, margin, plain=False):
    """None for a record that is invalid or not admissible at its transform; else (N, v, See, n, pivot) there."""
    height, width = labels.shape
    bx, by = CR.frame(T, W, H, width, height)
    s = MC.segments(keys, T, W, H, templates, rec, base)
    if s is None or not s[0]:
        return None
    _, ends, bins, posed = s
    ends = ends - np.array([[bx], [by], [bx], [by]], dtype=np.int64)
    S = (moments_plain if plain else moments)(labels, len(keys), ends, bins, MC.window(templates, rec, base, margin, width, height), radius, tol)
    return normal_equations(S, ends, float_ends(posed, T, bx, by))


def fit(labels, keys, T, W, H, templates, recs, base=0, radius=3, bin_tolerance=1, margin=None, iterations=2, min_pixels=8,
        damping=1e-3, max_shift=None, max_angle=0.1, plain=False):
    """(records, info (n, 4) int32, rms (n, 2) float32) of fdcm_matches_fit.  plain: the moments by moments_plain."""
    labels = np.asarray(labels)
    assert labels.ndim == 2 and labels.dtype == np.uint8
    keys = np.asarray(keys, dtype=np.float32)
    margin = radius if margin is None else margin
    par = dict(damping=damping, max_shift=radius if max_shift is None else max_shift, max_angle=max_angle)
    assert 1 <= iterations <= 8 and min_pixels >= 3 and 0 <= radius <= 32 and 0 <= bin_tolerance <= len(keys) // 2
    out = np.array(recs, dtype=MR.MATCH_DTYPE)
    info = np.zeros((len(out), 4), dtype=np.int32)
    rms = np.full((len(out), 2), np.nan, dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(len(out)):
            rec, prev, status, steps = out[j:j + 1].copy()[0], None, 0, 0
            for p in range(iterations + 1):
                here = pass_of(labels, keys, T, W, H, templates, rec, base, radius, bin_tolerance, margin, plain)
                if here is None:
                    if p == 0:
                        status = -1
                    else:   # the step leaves the map: not taken
                        rec["transform"], status, steps = prev, 4, steps - 1
                    break
                N, v, See, n, c = here
                if p == 0:
                    info[j, 2], rms[j, 0] = n, rms_of(See, n)
                info[j, 3], rms[j, 1] = n, rms_of(See, n)
                if p == iterations:
                    break
                if n < min_pixels:
                    status = 1
                    break
                status, x0, x1, x2 = solve_step(N, v, par)
                if status:
                    break
                new = fold(rec["transform"], x0, x1, x2, c)
                if not np.all(np.isfinite(new)):
                    status = 2
                    break
                prev = rec["transform"].copy()
                if not (x0 == 0 and x1 == 0 and x2 == 0):
                    rec["transform"] = new
                steps += 1
            out[j]["transform"] = rec["transform"]
            info[j, 0], info[j, 1] = status, steps
    return out, info, rms
