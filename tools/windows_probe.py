"""One fixed pose-window search, for comparing the library's paths: prints the SHA-256 of the records and offsets.

    python tools/windows_probe.py                          the default path
    FDCM_WINDOWS_BATCH=5 python tools/windows_probe.py     batches of 5 planes at most: dozens of batches
    FDCM_WINDOWS_FLAT=1 python tools/windows_probe.py      64-bit flat addresses

The digests must be equal (tests/test_gpu_exhaustive_windows.py runs the three in fresh processes: the switches are read
once per process)."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def case():
    """(scene, templates, cs, pivots, [(jobs, (sx, sy), wrap, k)])"""
    from openfdcm_amd import synthetic
    scene = synthetic.scene(256, 48, 9)
    rng = np.random.default_rng(61)
    tmpls = []
    for n in (0, 5, 12, 23):
        c = rng.uniform(75, 180, size=2)
        tmpls.append((c[:, None] + rng.uniform(-50, 50, size=(2, 2 * n))).astype(np.float32).reshape(4, n, order="F"))
    a = np.deg2rad([0, 20, 45, 90, 135, 180, 250, 330])
    cs = np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)
    piv = np.float32([[0, 0], [120, 130], [128.5, 127.25], [131, 119]])
    jobs = []
    for q in range(72):
        nx, ny = [(1, 1), (3, 3), (5, 2), (17, 65), (64, 16), (9, 9)][q % 6]
        a0, na = [(0, 1), (0, 8), (6, 4), (3, 1), (2, 5), (7, 3), (5, 2)][q % 7]
        jobs.append((q % 4, a0, na, int(rng.integers(-190, -20)), int(rng.integers(-180, -20)), nx, ny))
    jobs = np.asarray(jobs, dtype=np.int32)
    return scene, tmpls, cs, piv, [(jobs, (1, 1), True, 8), (jobs, (2, 3), True, 64), (jobs[jobs[:, 1] + jobs[:, 2] <= 8], (1, 1), False, 1)]


def run():
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    scene, tmpls, cs, piv, calls = case()
    dev = DeviceFeatureMap.build(scene, depth=12, coeff=5.0, padding=1.2, distance=0)
    tset = DeviceTemplates(tmpls)
    h = hashlib.sha256()
    n = 0
    for jobs, (sx, sy), wrap, k in calls:
        rec, off = dev.exhaustive_window_search(tset, jobs, cs, piv, sx=sx, sy=sy, wrap=wrap, k=k)
        h.update(rec.tobytes())
        h.update(off.tobytes())
        n += len(rec)
    rec, off = dev.exhaustive_window_search(tset, [(j[0], 0, 1, j[3], j[4], j[5], j[6]) for j in calls[0][0]], k=4)
    h.update(rec.tobytes())
    h.update(off.tobytes())
    return h.hexdigest(), n + len(rec)


if __name__ == "__main__":
    digest, n = run()
    print(f"windows_probe {digest} records {n}")
