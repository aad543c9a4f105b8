"""One fixed set of scene coverage and selection calls on match records (include/fdcm.h, "Match lists: scene coverage and
selection"), for comparing the library's paths: prints the SHA-256 of the counts, the residuals, the selected positions and
their counts.

    python tools/match_coverage_probe.py [n]                        the default path, on n records (700)
    FDCM_FORCE_HOST_BINS=1 python tools/match_coverage_probe.py     the bins from the host libm
    FDCM_MATCHED_FLAT=1 python tools/match_coverage_probe.py        the verify pass with 64-bit flat addresses (the table pass reads no volume)
    FDCM_COVERAGE_PART=300 python tools/match_coverage_probe.py     scene coverage in parts of 300 records
    FDCM_POISON=0 / FDCM_POISON=1 python tools/match_coverage_probe.py   the coverage buffers filled with the word before every call

The digests must be equal (tests/test_gpu_match_coverage.py runs the others in fresh processes, one after another: the
switches are read once per process)."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def case(n=700):
    """(labels, border, depth, templates, records)"""
    from openfdcm_amd import _capi
    rng = np.random.default_rng(97)
    width, height, border, depth = 96, 80, 5, 30
    labels = np.where(rng.random((height, width)) < 0.12, rng.integers(0, depth, size=(height, width)), 255).astype(np.uint8)
    tmpls = []
    for k in (0, 3, 9, 70, 300):
        c = rng.uniform(6, 24, size=(2, k))
        d = rng.uniform(-5, 5, size=(2, k))
        tmpls.append(np.concatenate([c - d, c + d]).astype(np.float32))
    r = np.zeros(n, dtype=_capi.MATCH_DTYPE)
    a = rng.uniform(-np.pi, np.pi, size=n)
    r["tmpl_idx"] = rng.integers(-1, len(tmpls) + 1, size=n)        # some out of range
    r["score"] = rng.uniform(0, 30, size=n)
    r["transform"] = np.stack([np.cos(a), -np.sin(a), rng.uniform(-10, width + 10, size=n), np.sin(a), np.cos(a),
                               rng.uniform(-10, height + 10, size=n)], axis=1)
    r["transform"][::37, 1] = np.nan
    r[5::50] = r[4:-1:50]                                           # duplicates
    return labels, border, depth, tmpls, r


def run(n=700):
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    labels, border, depth, tmpls, recs = case(n)
    dev = DeviceFeatureMap.build_labels(labels, border=border, depth=depth)
    tset = DeviceTemplates(tmpls)
    h = hashlib.sha256()
    admissible = accepted = 0
    for radius, tol in ((0, 0), (2, 1), (32, depth // 2)):
        counts, res = dev.match_coverage(labels, tset, recs, radius=radius, bin_tolerance=tol, residual=True)
        h.update(counts.tobytes())
        h.update(res.tobytes())
        admissible += int((counts[:, 0] >= 0).sum())
        for kw in (dict(min_new=0.5), dict(min_coverage=0.1, min_new=0.0, min_pixels=3, max_selected=70)):
            sel, c3, res = dev.select_matches(labels, tset, recs, radius=radius, bin_tolerance=tol, residual=True, **kw)
            for part in (sel, c3, res):
                h.update(part.tobytes())
            accepted += len(sel)
    return h.hexdigest(), admissible, accepted


if __name__ == "__main__":
    digest, admissible, accepted = run(int(sys.argv[1]) if len(sys.argv) > 1 else 700)
    print(f"match_coverage_probe {digest} admissible {admissible} accepted {accepted}")
