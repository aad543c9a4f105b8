"""One fixed set of calls of the detections over pose windows, for comparing the library's paths: prints the SHA-256 of the
records, boxes, fractions and job indices.

    python tools/window_detect_probe.py                        the default path
    FDCM_MATCHED_FLAT=1 python tools/window_detect_probe.py    64-bit flat addresses in the scoring, the winners' pass and
                                                               the fractions
    FDCM_WINDOWS_BATCH=5 python tools/window_detect_probe.py   the job list scored in many parts

The digests must be equal (tests/test_gpu_detect_windows.py runs the switches in fresh processes: they are read once per
process).  case() is also the main case of that test: a 96 x 80 map with planted template instances, six small templates
(one without lines, one with a line of length zero), twelve angles and about 200 jobs."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEG = np.arange(12) * 30.0
LINES = [5, 0, 3, 8, 6, 4]   # lines per template
TAU = 3.0                    # the scalar line cap
MASTER = (-30, -30, 150, 130)  # a stride-1 grid (x0, y0, nx, ny) that holds every job's window
WIDTH, HEIGHT = 96, 80


def angles():
    return np.deg2rad(DEG)


def cs_table():
    a = angles()
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)


def templates():
    rng = np.random.default_rng(41)
    out = []
    for t, n in enumerate(LINES):
        p = rng.uniform(0, 16, size=(2, 2 * n)).astype(np.float32).reshape(4, n, order="F")
        if t == 4:
            p[2:, 1] = p[:2, 1]  # a line of length zero
        out.append(np.ascontiguousarray(p))
    return out


def pivots(tmpls):
    out = np.zeros((len(tmpls), 2), dtype=np.float32)
    for t, tm in enumerate(tmpls):
        if tm.shape[1]:
            xs, ys = np.concatenate([tm[0], tm[2]]), np.concatenate([tm[1], tm[3]])
            out[t] = [(xs.min() + xs.max()) / np.float32(2), (ys.min() + ys.max()) / np.float32(2)]
    return out


def _rotate(lines, c, s, px, py):
    """The library's M_a in float32, left to right."""
    c, s, px, py = np.float32(c), np.float32(s), np.float32(px), np.float32(py)
    ns = -s
    mx, my = px - (c * px + ns * py), py - (s * px + c * py)
    out = np.empty_like(lines)
    for k in (0, 2):
        out[k] = (c * lines[k] + ns * lines[k + 1]) + mx
        out[k + 1] = (s * lines[k] + c * lines[k + 1]) + my
    return out


PLANTS = [(0, 2, 14, 10), (0, 7, 60, 12), (2, 0, 36, 8), (2, 5, 78, 30), (3, 3, 12, 38), (3, 10, 50, 40), (4, 1, 30, 56),
          (4, 8, 70, 58), (5, 4, 8, 60), (5, 11, 44, 22), (0, 9, 28, 34), (3, 6, 74, 6)]  # (tmpl, angle, tx, ty)


def case():
    """(scene, templates, cs, pivots, jobs)"""
    from openfdcm_amd import synthetic
    tmpls = templates()
    cs, piv = cs_table(), pivots(tmpls)
    base = synthetic.scene(WIDTH, 40, 5)[:, 2:]
    base = base[:, (base[1] <= HEIGHT - 1) & (base[3] <= HEIGHT - 1)]
    parts = [np.float32([[0, 0, 12, 0], [WIDTH - 1, HEIGHT - 1, WIDTH - 13, HEIGHT - 1]]).T, base[:, :14]]
    for t, a, tx, ty in PLANTS:
        inst = _rotate(tmpls[t], cs[a, 0], cs[a, 1], piv[t, 0], piv[t, 1]) + np.float32([tx, ty, tx, ty])[:, None]
        parts.append(np.clip(inst, [[0], [0], [0], [0]], [[WIDTH - 1], [HEIGHT - 1], [WIDTH - 1], [HEIGHT - 1]]).astype(np.float32))
    scene = np.ascontiguousarray(np.concatenate(parts, axis=1), dtype=np.float32)
    rng = np.random.default_rng(77)
    n = len(DEG)
    jobs = []
    for t, a, tx, ty in PLANTS:  # around the planted poses: the pose itself, neighbours that overlap it, a view next to it
        jobs.append((t, (a - 1) % n, 3, tx - 2, ty - 2, 5, 5))
        jobs.append((t, a, 1, tx + 1, ty - 3, 4, 6))
        jobs.append(((t + 1) % len(LINES), (a - 1) % n, 2, tx - 1, ty - 1, 3, 3))
    jobs += [jobs[0], jobs[4], jobs[0]]                                   # duplicates
    jobs += [(0, 10, 4, 40, 30, 6, 5), (3, 11, 3, 20, 20, 5, 5)]          # runs that cross the end of the table
    jobs += [(2, 0, 4, -25, -28, 128, 128)]                               # the 65 536 limit
    jobs += [(5, 3, 2, -29, 10, 6, 6), (4, 0, 1, 100, 90, 9, 9), (0, 6, 1, -12, -14, 16, 17), (3, 2, 2, 84, 66, 12, 14)]  # outside, across
    for _ in range(40):                                                   # one-point jobs
        jobs.append((int(rng.integers(0, len(LINES))), int(rng.integers(0, n)), 1, int(rng.integers(-8, 90)), int(rng.integers(-8, 74)), 1, 1))
    while len(jobs) < 204:
        nx, ny = [(3, 3), (5, 5), (7, 5), (4, 17), (9, 2)][int(rng.integers(0, 5))]
        jobs.append((int(rng.integers(0, len(LINES))), int(rng.integers(0, n)), int(rng.integers(1, 5)), int(rng.integers(-10, 86)),
                     int(rng.integers(-10, 70)), nx, ny))
    return scene, tmpls, cs, piv, np.asarray(jobs, dtype=np.int32)


def build(scene):
    """The 96 x 80 map: a built map is square (96 x 96, the scene moved down by 8), so the rows the scene occupies are
    adopted as a map of their own with scene translation (0, 0)."""
    from openfdcm_amd.engine import DeviceFeatureMap
    full = DeviceFeatureMap.build(scene, depth=12, coeff=5.0, padding=1.0, distance=0)
    tx, ty = (float(v) for v in full.scene_translation)
    assert (full.width, full.height) == (WIDTH, WIDTH) and tx == 0 and ty == (WIDTH - HEIGHT) // 2
    vol = full.volume()[:, :, int(ty):int(ty) + HEIGHT]
    return DeviceFeatureMap.from_volume(full.keys, vol, (0.0, 0.0))


CALLS = [dict(overlap_permille=300, min_matched=0.5, max_score=2.0), dict(overlap_permille=0, min_matched=None, max_score=float("inf")),
         dict(overlap_permille=1000, min_matched=0.25, max_score=float("inf")), dict(overlap_permille=300, min_matched=None, max_score=1.0)]


def run():
    from openfdcm_amd.engine import DeviceTemplates
    scene, tmpls, cs, piv, jobs = case()
    dev = build(scene)
    h = hashlib.sha256()
    n = 0
    for tset in (DeviceTemplates(tmpls, line_caps=TAU), DeviceTemplates(tmpls)):
        for kw in CALLS:
            for c, pv, jb in [(cs, piv, jobs), (None, None, np.concatenate([jobs[:, :1], 0 * jobs[:, :1], 0 * jobs[:, :1] + 1, jobs[:, 3:]], axis=1))]:
                got = dev.exhaustive_detect_windows(tset, jb, c, pv, wrap=True, max_detections=100, margin=1, penalty=0, boxes=True,
                                                    matched=True, job_index=True, **kw)
                for part in got:
                    h.update(np.ascontiguousarray(part).tobytes())
                n += len(got[0])
    return h.hexdigest(), n


if __name__ == "__main__":
    digest, n = run()
    print(f"window_detect_probe {digest} records {n}")
