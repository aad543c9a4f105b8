"""The numpy definition of fdcm_matches_refine (include/fdcm.h, "Match lists: refinement"), its referee.  Not collected: the
tests import it.  It works on a volume [k][x][y], the keys and the scene translation, and never calls the kernels it judges.

The lines of run position e are rotation_ref.rotate_lines of the record's template by (c, s) = cs[e] about its pivot (the
lines as they are with cs None), posed by match_ref.posed; the bin of a posed line is pyoracle.closest_orientation of the
posed, untranslated line.  The score of (r, e, i, j) is what match_ref.costs_of and pyoracle.eigen_sum give for those lines
with the offset float32(T + float32(i sx)), float32(T + float32(j sy)) in the scene translation's place, the costs clamped to
the caps; `window` computes all poses of a plane at once with the same float32 operations (costs_of's and eigen_sum's,
array-wide: test_refine_definition.py holds it against the two, pose by pose).  Keys are Python integers."""
import numpy as np

import match_ref as R
import rotation_ref as ROT
from oracle import pyoracle as P

f32 = np.float32
NAN = f32(np.nan)


def eigen_sum_rows(c):
    """pyoracle.eigen_sum of every row of a (poses, n) float32 array: the same packets, the same order."""
    c = np.asarray(c, dtype=np.float32)
    n = c.shape[1]
    if n == 0:
        return np.zeros(c.shape[0], dtype=np.float32)
    a2, a1 = (n // 8) * 8, (n // 4) * 4
    with np.errstate(all="ignore"):
        if a1:
            p0 = c[:, 0:4].copy()
            if a1 > 4:
                p1 = c[:, 4:8].copy()
                for i in range(8, a2, 8):
                    p0 = p0 + c[:, i:i + 4]
                    p1 = p1 + c[:, i + 4:i + 8]
                p0 = p0 + p1
                if a1 > a2:
                    p0 = p0 + c[:, a2:a2 + 4]
            res = (p0[:, 0] + p0[:, 2]) + (p0[:, 1] + p0[:, 3])
            start = a1
        else:
            res = c[:, 0].copy()
            start = 1
        for i in range(start, n):
            res = res + c[:, i]
    return res.astype(np.float32)


def offsets(t, h, s):
    """float32(T + float32(i s)) for i = -h .. h."""
    return np.array([f32(f32(t) + f32(i * s)) for i in range(-h, h + 1)], dtype=np.float32)


def run_lines(templates, cs, pivots):
    """sets[e][t]: the (4, n) lines Q_e(t); cs None: one run position, the lines as they are."""
    base = [R.lines_of(templates, t) for t in range(len(templates))]
    if cs is None:
        return [base]
    cs = np.asarray(cs, dtype=np.float32).reshape(-1, 2)
    return [[ROT.rotate_lines(tm, c, s, *((0.0, 0.0) if pivots is None else pivots[t])) for t, tm in enumerate(base)] for c, s in cs]


def window(vol, keys, t, p, cap, hx, hy, sx, sy):
    """The scores of the posed lines p (4, n) at every translation of the window: (2 hy + 1, 2 hx + 1) float32, and the mask of
    the admissible ones.  A score where the pose is not admissible means nothing."""
    W, H = vol.shape[1], vol.shape[2]
    n = p.shape[1]
    nx, ny = 2 * hx + 1, 2 * hy + 1
    ox, oy = offsets(t[0], hx, sx), offsets(t[1], hy, sy)
    with np.errstate(all="ignore"):
        X = (p[[0, 2]][None] + ox[:, None, None]).astype(np.float32)          # (nx, 2, n)
        Y = (p[[1, 3]][None] + oy[:, None, None]).astype(np.float32)
        okx = np.all((X > f32(-1)) & (X < f32(W)), axis=(1, 2))                # a NaN fails
        oky = np.all((Y > f32(-1)) & (Y < f32(H)), axis=(1, 2))
    adm = oky[:, None] & okx[None, :]
    scores = np.full((ny, nx), NAN, dtype=np.float32)
    I, J = np.flatnonzero(okx), np.flatnonzero(oky)
    if len(I) == 0 or len(J) == 0:
        return scores, adm
    bins = np.array([P.closest_orientation(keys, p[:, i]) for i in range(n)], dtype=np.int64)
    xi, yj = X[I].astype(np.int64), Y[J].astype(np.int64)                      # truncation
    with np.errstate(all="ignore"):
        a = vol[bins[None, None, :], xi[None, :, 0, :], yj[:, None, 0, :]]    # (nj, ni, n)
        b = vol[bins[None, None, :], xi[None, :, 1, :], yj[:, None, 1, :]]
        c = np.abs((a - b).astype(np.float32))
        c = np.where(c > cap[None, None, :], cap[None, None, :], c).astype(np.float32)
    scores[np.ix_(J, I)] = eigen_sum_rows(c.reshape(-1, n)).reshape(len(J), len(I))
    return scores, adm


def pose_score(vol, keys, t, p, cap, tau):
    """One pose by match_ref.costs_of and pyoracle.eigen_sum: (admissible, score) of the lines p at translation tau."""
    off = (f32(f32(t[0]) + f32(tau[0])), f32(f32(t[1]) + f32(tau[1])))
    adm, c = R.costs_of(vol, keys, off, p)
    if not adm:
        return False, NAN
    with np.errstate(all="ignore"):
        return True, P.eigen_sum(np.where(c > cap, cap, c).astype(np.float32))


def refined_transform(M, cs, pivot, e, i, j, sx, sy):
    """M' of the pose (e, i, j) for the record's M (6 float32)."""
    M = np.asarray(M, dtype=np.float32)
    fx, fy = f32(i * sx), f32(j * sy)
    out = M.copy()
    with np.errstate(all="ignore"):
        if cs is None:
            out[2], out[5] = f32(M[2] + fx), f32(M[5] + fy)
            return out
        c, s = np.asarray(cs, dtype=np.float32).reshape(-1, 2)[e]
        Q = ROT.rot_matrix(c, s, *pivot)
        ns, mx, my = Q[0, 1], Q[0, 2], Q[1, 2]
        out[0] = f32(f32(M[0] * c) + f32(M[1] * s))
        out[1] = f32(f32(M[0] * ns) + f32(M[1] * c))
        out[2] = f32(f32(f32(f32(M[0] * mx) + f32(M[1] * my)) + M[2]) + fx)
        out[3] = f32(f32(M[3] * c) + f32(M[4] * s))
        out[4] = f32(f32(M[3] * ns) + f32(M[4] * c))
        out[5] = f32(f32(f32(f32(M[3] * mx) + f32(M[4] * my)) + M[5]) + fy)
    return out


def refine(vol, keys, t, templates, recs, base=0, cs=None, pivots=None, centre=-1, hx=0, hy=0, sx=1, sy=1, caps=None):
    """(records, poses (n, 3) int32, partial (n,) bool) of fdcm_matches_refine; partial: some but not all poses of the record's
    window are admissible."""
    vol = np.asarray(vol, dtype=np.float32)
    caps = R.flat_caps(templates, caps)
    sets = run_lines(templates, cs, pivots)
    nx, ny = 2 * hx + 1, 2 * hy + 1
    N = nx * ny
    out = np.array(recs, dtype=R.MATCH_DTYPE)
    out["score"] = NAN
    poses = np.zeros((len(recs), 3), dtype=np.int32)
    poses[:, 0] = -1
    partial = np.zeros(len(recs), dtype=bool)
    for r, rec in enumerate(recs):
        ti = int(rec["tmpl_idx"]) - base
        if not 0 <= ti < len(templates) or R.lines_of(templates, ti).shape[1] == 0:
            continue
        best, n_adm = None, 0
        for e, tm in enumerate(sets):
            p = R.posed(tm, rec, base)
            s, adm = window(vol, keys, t, p, caps[ti], hx, hy, sx, sy)
            n_adm += int(adm.sum())
            bits = s.view(np.uint32)
            for jj, ii in zip(*np.nonzero(adm & ~np.isnan(s))):
                centre_pose = e == centre and ii == hx and jj == hy
                key = (int(bits[jj, ii]) << 32) | (0 if centre_pose else 1 + e * N + int(jj) * nx + int(ii))
                if best is None or key < best[0]:
                    best = (key, e, int(ii) - hx, int(jj) - hy)
        partial[r] = 0 < n_adm < len(sets) * N
        if best is None:
            continue
        key, e, i, j = best
        out["score"][r] = np.array([key >> 32], dtype=np.uint32).view(np.float32)[0]
        out["transform"][r] = refined_transform(rec["transform"], cs, (0.0, 0.0) if pivots is None else pivots[ti], e, i, j, sx, sy)
        poses[r] = (e, i, j)
    return out, poses, partial
