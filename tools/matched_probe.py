"""One fixed set of calls by matched fraction, for comparing the library's paths: prints the SHA-256 of the records, boxes and
fractions.

    python tools/matched_probe.py                        the default path
    FDCM_MATCHED_FLAT=1 python tools/matched_probe.py    64-bit flat addresses

The digests must be equal (tests/test_gpu_matched.py runs the second in a fresh process: the switch is read once per
process)."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def case():
    """(scene, templates, caps tau, cs, pivots, grids)"""
    from openfdcm_amd import synthetic
    scene = synthetic.scene(256, 48, 9)
    rng = np.random.default_rng(67)
    tmpls = []
    for n in (0, 3, 9, 70):
        c = rng.uniform(110, 150, size=2)
        tmpls.append((c[:, None] + rng.uniform(-40, 40, size=(2, 2 * n))).astype(np.float32).reshape(4, n, order="F"))
    a = np.deg2rad([0, 45, 250])
    cs = np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)
    piv = np.float32([[0, 0], [120, 130], [128.5, 127.25], [131, 119]])
    return scene, tmpls, 3.0, cs, piv, [(-95, -100, 37, 70, 1, 1), (-120, -130, 37, 70, 3, 2)]


def run():
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    scene, tmpls, tau, cs, piv, grids = case()
    dev = DeviceFeatureMap.build(scene, depth=12, coeff=5.0, padding=1.2, distance=0)
    tset = DeviceTemplates(tmpls, line_caps=tau)
    h = hashlib.sha256()
    n = gated = 0
    for grid in grids:
        for c, pv in [(None, None), (cs, piv)]:
            A = 1 if c is None else len(c)
            for mm in (0.0, 0.4, 0.7):
                rec, box, fr = dev.exhaustive_detect_all(tset, grid, c, pv, max_detections=200, overlap_permille=300, margin=1, penalty=0,
                                                         min_matched=mm, boxes=True, matched=True)
                for part in (rec, box, fr):
                    h.update(part.tobytes())
                n += len(rec)
                gated += mm > 0 and len(rec) > 0
            # the poses of the grid's points for every pair, admissible or not
            x0, y0, nx, ny, sx, sy = grid
            xs, ys = np.meshgrid(x0 + sx * np.arange(0, nx, 5), y0 + sy * np.arange(0, ny, 7))
            poses = np.array([(t, a, x, y) for t in range(len(tmpls)) for a in range(A) for x, y in zip(xs.ravel(), ys.ravel())],
                             dtype=np.int32)
            fr = dev.matched_fractions(tset, poses, c, pv)
            h.update(fr.tobytes())
            n += int(np.isfinite(fr).sum())
    return h.hexdigest(), n, int(gated)


if __name__ == "__main__":
    digest, n, gated = run()
    print(f"matched_probe {digest} values {n} gated {gated}")
