"""The numpy statement of the detections over pose windows (include/fdcm.h, "Detections over pose windows"), the referee of
fdcm_search_exhaustive_detect_windows.  Not collected: the tests import it.

Inputs are planes other tests hold to their definitions: per template its (A, NY, NX) score volume on a stride-1 master grid
(rotation_score_map / score_map of the set with its caps: NaN where not admissible) and, for the gate and the fractions, the
uncapped cost maps of its lines on the same grid (capped_ref.line_cost_maps, the floats of fdcm_line_costs).

  winner of job j   the smallest key (score bits << 32) | (e N_j + g) over the job's run positions e and grid points g whose
                    score is not NaN; none when there is no such point (or the template has no lines)
  q_j               float32(score / den[tmpl]), one division
  ML, need, frac    matched_ref's rules on the line costs at the winner's pose
  candidates        jobs with a winner, q not NaN, q <= max_score, ML >= need
  key(j)            (bits of q_j << 32) | j;  F(j) = box[tmpl, a_j] + t_j
  greedy rule       in Python integers: the candidate of the smallest key is a detection; it and every candidate with
                    1000 I > permille U against it leave; until none is left or max_detections is reached"""
import numpy as np

from matched_ref import fractions, matched_lengths, need as need_of
from rotation_ref import rot_matrix
from windows_ref import job_volume

f32 = np.float32


def winners(vols, master, jobs, n, sx, sy):
    """Per job (e, g, score) of its winner, or None."""
    out = []
    for job in np.asarray(jobs).reshape(-1, 7):
        tmpl = int(job[0])
        if vols[tmpl] is None:
            out.append(None)
            continue
        v = np.ascontiguousarray(job_volume(vols[tmpl], master, job, n, sx, sy), dtype=np.float32).reshape(-1)
        ok = ~np.isnan(v)
        if not ok.any():
            out.append(None)
            continue
        key = (v.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(v.size, dtype=np.uint64)
        i = int(np.argmin(np.where(ok, key, np.uint64(2 ** 64 - 1))))
        N = int(job[5]) * int(job[6])
        out.append((i // N, i % N, v[i]))
    return out


def detect_windows_ref(vols, master, jobs, cs, pivots, sx, sy, den, boxes, max_score, max_detections, permille, min_matched=0.0,
                       costs=None, caps=None, lens=None, base=0):
    """(records, boxes (n, 4) int32, fractions (n,) float32, jobs (n,) int32, counts) of the call.  den: (T,) float32
    denominators; boxes: (T, A, 4) footprints at the call's margin; costs[t]: (lines, A, NY, NX) uncapped line cost maps on
    master, caps[t] and lens[t] the lines' caps and lengths (needed for the gate and the fractions; None: fractions NaN, no
    gate allowed).  counts: jobs without a winner, removed by the threshold, by the gate, by suppression, and detections."""
    from openfdcm_amd import _capi
    jobs = np.asarray(jobs).reshape(-1, 7)
    n = 1 if cs is None else len(cs)
    X0, Y0 = master[0], master[1]
    W = winners(vols, master, jobs, n, sx, sy)
    cand = {}  # job -> (key, F, q, a, tx, ty, frac)
    counts = dict(no_winner=0, threshold=0, gate=0, suppressed=0, detections=0)
    for j, w in enumerate(W):
        if w is None:
            counts["no_winner"] += 1
            continue
        tmpl, a0, na, x0, y0, nx, ny = (int(v) for v in jobs[j])
        e, g, s = w
        a = (a0 + e) % n
        tx, ty = x0 + (g % nx) * sx, y0 + (g // nx) * sy
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            q = f32(s) / f32(den[tmpl])
        if np.isnan(q) or not q <= f32(max_score):
            counts["threshold"] += 1
            continue
        frac = f32(np.nan)
        if costs is not None:
            c = costs[tmpl][:, a, ty - Y0, tx - X0]
            ml = matched_lengths(c, caps[tmpl], lens[tmpl])
            tl = matched_lengths(np.zeros_like(c), np.full(len(c), np.inf, dtype=np.float32), lens[tmpl])  # every line matched
            frac = fractions(ml, tl)
            if not ml >= need_of(min_matched, tl):
                counts["gate"] += 1
                continue
        else:
            assert min_matched == 0
        b = [int(v) for v in boxes[tmpl, a]]
        key = (int(np.asarray(q, dtype=np.float32).view(np.uint32)) << 32) | j
        cand[j] = (key, (b[0] + tx, b[1] + ty, b[2] + tx, b[3] + ty), q, a, tx, ty, frac)
    n_cand = len(cand)
    out = []
    while len(out) < max_detections and cand:
        d = min(cand, key=lambda j: cand[j][0])
        D = cand.pop(d)
        out.append((d, D))
        for j in list(cand):
            G, F = cand[j][1], D[1]
            inter = max(0, min(G[2], F[2]) - max(G[0], F[0]) + 1) * max(0, min(G[3], F[3]) - max(G[1], F[1]) + 1)
            union = (G[2] - G[0] + 1) * (G[3] - G[1] + 1) + (F[2] - F[0] + 1) * (F[3] - F[1] + 1) - inter
            if 1000 * inter > permille * union:
                del cand[j]
    counts["detections"] = len(out)
    counts["suppressed"] = n_cand - len(out) - len(cand)
    rec = np.zeros(len(out), dtype=_capi.MATCH_DTYPE)
    F = np.zeros((len(out), 4), dtype=np.int32)
    fr = np.zeros(len(out), dtype=np.float32)
    ji = np.zeros(len(out), dtype=np.int32)
    for l, (j, (key, box, q, a, tx, ty, frac)) in enumerate(out):
        tmpl = int(jobs[j][0])
        rec["tmpl_idx"][l] = tmpl + base
        rec["score"][l] = q
        if cs is None:
            rec["transform"][l] = [1, 0, f32(tx), 0, 1, f32(ty)]
        else:
            px, py = (0.0, 0.0) if pivots is None else pivots[tmpl]
            M = rot_matrix(cs[a][0], cs[a][1], px, py)
            rec["transform"][l] = [M[0, 0], M[0, 1], M[0, 2] + f32(tx), M[1, 0], M[1, 1], M[1, 2] + f32(ty)]
        F[l], fr[l], ji[l] = box, frac, j
    return rec, F, fr, ji, counts
