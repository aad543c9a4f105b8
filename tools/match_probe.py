"""One fixed set of calls on match lists (include/fdcm.h, "Match lists"), for comparing the library's paths: prints the SHA-256
of the scores, fractions, line costs, records, positions, boxes and matched fractions.

    python tools/match_probe.py                            the default path
    FDCM_MATCHED_FLAT=1 python tools/match_probe.py        64-bit flat addresses
    FDCM_FORCE_HOST_BINS=1 python tools/match_probe.py     the bins from the host libm
    FDCM_POISON=0 / FDCM_POISON=1 python tools/match_probe.py   the workspace filled with the word before every call

The digests must be equal (tests/test_gpu_matches.py runs the others in fresh processes, one after another: the switches are
read once per process)."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def case():
    """(scene, adopted (keys, volume, translation), templates, records per map)"""
    from openfdcm_amd import _capi, synthetic
    rng = np.random.default_rng(311)
    tmpls = []
    for n in (0, 3, 9, 70, 130):
        c = rng.uniform(4, 20, size=(2, n))
        d = rng.uniform(-4, 4, size=(2, n))
        tmpls.append(np.concatenate([c - d, c + d]).astype(np.float32))
    keys = (np.arange(6) * np.pi / 6 - np.pi / 2).astype(np.float32)
    vol = (rng.random((6, 70, 37)) * 50).astype(np.float32)
    vol[1, 20:24, 10:14] = np.nan
    vol[3, 40:44, 20:24] = np.inf

    def records(W, H, n):
        r = np.zeros(n, dtype=_capi.MATCH_DTYPE)
        a = rng.uniform(-np.pi, np.pi, size=n)
        r["tmpl_idx"] = rng.integers(-1, len(tmpls) + 1, size=n)        # some out of range
        r["score"] = np.round(rng.uniform(0, 30, size=n))               # ties
        r["transform"] = np.stack([np.cos(a), -np.sin(a), rng.uniform(0, W, size=n), np.sin(a), np.cos(a), rng.uniform(0, H, size=n)], axis=1)
        r["transform"][::37, 1] = np.nan
        r[5::50] = r[4:-1:50]                                           # duplicates
        return r
    return synthetic.scene(90, 24, 11), (keys, vol, np.float32([3.5, -2.25])), tmpls, records


def run():
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    scene, (keys, vol, tr), tmpls, records = case()
    maps = [DeviceFeatureMap.build(scene, depth=12, coeff=5.0, padding=1.3, distance=0), DeviceFeatureMap.from_volume(keys, vol, tr)]
    h = hashlib.sha256()
    values = kept = 0
    for dev in maps:
        recs = records(dev.width, dev.height, 600)
        for caps in (None, 2.0):
            tset = DeviceTemplates(tmpls, line_caps=caps)
            s, f, c = dev.verify_matches(tset, recs)
            for part in (s, f, c):
                h.update(np.where(np.isnan(part), np.float32(np.nan), part).tobytes())
            values += int(np.isfinite(s).sum())
            for kw in (dict(penalty=0, overlap_permille=300), dict(overlap_permille=1000, max_detections=200, rescore=True),
                       dict(penalty=0, overlap_permille=0, min_matched=0.4, max_score=6.0, margin=2, rescore=True)):
                res = dev.detect_matches(tset, recs, indices=True, boxes=True, matched=True, **kw)
                for part in res:
                    h.update(part.tobytes())
                kept += len(res[0])
    return h.hexdigest(), values, kept


if __name__ == "__main__":
    digest, values, kept = run()
    print(f"match_probe {digest} values {values} kept {kept}")
