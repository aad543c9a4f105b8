"""The numpy referee of fdcm_search_exhaustive_windows (include/fdcm.h, "Pose windows").  Not collected: the tests import it.

A job's answer is by definition fdcm_search_exhaustive_rotations' for its template alone, its run of rotations alone and its
grid: so the referee slices the (A, NY, NX) score volume of the job's template, given on a stride-1 master grid, on the
job's run and grid, and hands the slice to rotation_ref.peaks3 with radii 0.  Keys and their order are stated there only."""
import numpy as np

from rotation_ref import peaks3, rot_matrix

f32 = np.float32


def admissible_axis(p, off, size, ts):
    """Per integer translation of ts: -1 < fl(p + fl(off + t)) < size for every end point coordinate p (float32 sums)."""
    p = np.asarray(p, dtype=np.float32).reshape(-1, 1)
    v = p + (f32(off) + np.asarray(ts).astype(np.float32))[None, :]
    return np.all((v > f32(-1)) & (v < f32(size)), axis=0)


def admissible_mask(lines, scene_translation, width, height, master):
    """(NY, NX) bool: the admissible translations of the (4, N) line set on the stride-1 grid master = (X0, Y0, NX, NY)."""
    X0, Y0, NX, NY = master
    lines = np.asarray(lines, dtype=np.float32).reshape(4, -1)
    ax = admissible_axis(lines[[0, 2]], scene_translation[0], width, X0 + np.arange(NX))
    ay = admissible_axis(lines[[1, 3]], scene_translation[1], height, Y0 + np.arange(NY))
    return ay[:, None] & ax[None, :]


def job_volume(vol, master, job, n, sx, sy):
    """The (na, ny, nx) volume of one job: rotations (a0 + e) mod n and the job's grid points out of vol (A, NY, NX) on the
    master grid, which must contain the job's window."""
    X0, Y0, NX, NY = master
    tmpl, a0, na, x0, y0, nx, ny = (int(v) for v in job)
    cols, rows = x0 + sx * np.arange(nx) - X0, y0 + sy * np.arange(ny) - Y0
    assert cols[0] >= 0 and cols[-1] < NX and rows[0] >= 0 and rows[-1] < NY, "the job's window leaves the master grid"
    run = (a0 + np.arange(na)) % n
    return vol[run][:, rows][:, :, cols]


def window_records(vols, master, jobs, cs, pivots, k, sx, sy, wrap, base=0):
    """(records, offsets) of fdcm_search_exhaustive_windows.  vols[t]: template t's (A, NY, NX) volume on master, NaN where
    not admissible, or None for a template without lines; cs (A, 2) or None for the translations (A = 1)."""
    from openfdcm_amd import _capi
    jobs = np.asarray(jobs).reshape(-1, 7)
    n = 1 if cs is None else len(cs)
    out, offsets = [], [0]
    for job in jobs:
        tmpl, a0, na, x0, y0, nx, ny = (int(v) for v in job)
        r = np.zeros(0, dtype=_capi.MATCH_DTYPE)
        if vols[tmpl] is not None:
            e, g, s = peaks3(job_volume(vols[tmpl], master, job, n, sx, sy), k, 0, 0, 0, wrap)
            r = np.zeros(len(g), dtype=_capi.MATCH_DTYPE)
            r["tmpl_idx"] = tmpl + base
            r["score"] = s
            tr = np.zeros((len(g), 6), dtype=np.float32)
            for q in range(len(g)):
                tx, ty = f32(x0 + (g[q] % nx) * sx), f32(y0 + (g[q] // nx) * sy)
                if cs is None:
                    tr[q] = [1, 0, tx, 0, 1, ty]
                else:
                    a = (a0 + int(e[q])) % n
                    px, py = (0.0, 0.0) if pivots is None else pivots[tmpl]
                    M = rot_matrix(cs[a][0], cs[a][1], px, py)
                    tr[q] = [M[0, 0], M[0, 1], M[0, 2] + tx, M[1, 0], M[1, 1], M[1, 2] + ty]
            r["transform"] = tr
        out.append(r)
        offsets.append(offsets[-1] + len(r))
    rec = np.concatenate(out) if out else np.zeros(0, dtype=_capi.MATCH_DTYPE)
    return rec, np.asarray(offsets, dtype=np.int64)
