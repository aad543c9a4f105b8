"""One fixed set of scene coverage and selection calls on pose lists (include/fdcm.h, "Scene coverage", "Scene selection"), for
comparing the library's paths: prints the SHA-256 of the counts, the residuals, the selected indices and their counts.

    python tools/coverage_probe.py                                  the default path
    FDCM_POISON=0 / FDCM_POISON=1 python tools/coverage_probe.py    the coverage buffers filled with the word before every call

The digests must be equal (tests/test_gpu_coverage.py runs them in fresh processes, one after another: the switches are read
once per process).  The calls take host labels and device labels, with and without a residual, plain and with a table of 7
angles with pivots; the windows at radius 32 have more than one strip, and the selection crosses a batch of rounds."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEGREES = [0, 20, 45, 90, 135, 250, 330]


def case(n_rot):
    """(labels, border, depth, templates, poses) for a table of n_rot rotations"""
    rng = np.random.default_rng(131)
    width, height, border, depth = 96, 80, 5, 30
    labels = np.where(rng.random((height, width)) < 0.12, rng.integers(0, depth, size=(height, width)), 255).astype(np.uint8)
    tmpls = []
    for k in (0, 3, 9, 70, 300):                                    # 300: more than the kernel's LDS chunk of 256 segments
        c = rng.uniform(1.5, 3.5, size=(2, k)) if k == 3 else rng.uniform(6, 24, size=(2, k))
        d = rng.uniform(-1, 1, size=(2, k)) if k == 3 else rng.uniform(-5, 5, size=(2, k))
        tmpls.append(np.concatenate([c - d, c + d]).astype(np.float32))
    p = [[rng.integers(0, 5), rng.integers(0, n_rot), rng.integers(-border - 3, width - 8), rng.integers(-border - 3, height - 6)]
         for _ in range(270)]
    p += [[1, 0, -border, 10], [1, 0, 20, -border], [1, 0, width, 10], [1, 0, 20, height]]     # in the map's border: the window misses the image
    p += [[2, 0, -1000, 0], [3, 0, 0, 5000], [4, 0, width, 0], [2, n_rot - 1, (1 << 24) - 1, 0], [4, 0, -border - 9, 3]]   # not admissible
    p += [[3, 0, 20 + i, 6 + j] for i, j in [(0, 0), (1, 0), (0, 2), (3, 3), (0, 0)]]            # overlapping windows, a duplicate
    p += [p[3], p[7], p[31], p[100], p[271], p[275]]                                              # duplicates
    p += [[4, n_rot - 1, 12, 5], [4, 0, 12, 5], [0, 0, 5, 5], [0, n_rot // 2, 40, 40]]
    return labels, border, depth, tmpls, np.asarray(p, dtype=np.int32)


def run():
    import torch
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    h = hashlib.sha256()
    admissible = empty = most = calls = 0
    for rot in (False, True):
        labels, border, depth, tmpls, poses = case(7 if rot else 1)
        on_device = torch.from_numpy(labels).cuda()
        dev = DeviceFeatureMap.build_labels(labels, border=border, depth=depth)
        tset = DeviceTemplates(tmpls)
        ang = np.deg2rad(DEGREES)
        cs = np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32) if rot else None
        pv = fd.template_pivots(tmpls) if rot else None

        def add(*parts):
            for part in parts:
                h.update(np.ascontiguousarray(part.cpu().numpy() if hasattr(part, "cpu") else part).tobytes())

        for radius, tol, margin in ((0, 0, 0), (2, 1, None), (32, depth // 2, None)):
            kw = dict(cs=cs, pivots=pv, radius=radius, bin_tolerance=tol, margin=margin)
            for lab in (labels, on_device):
                counts = dev.scene_coverage(lab, tset, poses, **kw)
                again, res = dev.scene_coverage(lab, tset, poses, residual=True, **kw)
                assert np.array_equal(counts, again)
                add(counts, res)
                admissible += int((counts[:, 0] >= 0).sum())
                empty += int((counts[:, 0] == 0).sum())
                for ms in (1, 70, 4096):                            # min_new 0: every candidate with a pixel of its own is accepted
                    sel, c3, res = dev.scene_select(lab, tset, poses, min_coverage=0.0, min_new=0.0, min_pixels=1, max_selected=ms,
                                                    residual=True, **kw)
                    add(sel, c3, res)
                    most = max(most, len(sel))
                sel, c3 = dev.scene_select(lab, tset, poses, min_coverage=0.1, min_new=0.5, min_pixels=3, max_selected=70, **kw)
                add(sel, c3)
                calls += 6
    return h.hexdigest(), admissible, empty, most, calls


if __name__ == "__main__":
    digest, admissible, empty, most, calls = run()
    print(f"coverage_probe {digest} admissible {admissible} empty {empty} most {most} calls {calls}")
