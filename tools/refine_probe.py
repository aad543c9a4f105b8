"""One fixed set of calls of refine_matches (include/fdcm.h, "Match lists: refinement"), for comparing the library's paths: prints
the SHA-256 of the refined records and their poses.

    python tools/refine_probe.py                            the default path
    FDCM_MATCHED_FLAT=1 python tools/refine_probe.py        64-bit flat addresses
    FDCM_FORCE_HOST_BINS=1 python tools/refine_probe.py     the bins from the host libm
    FDCM_REFINE_PART=100 python tools/refine_probe.py       the list in parts of 100 records
    FDCM_POISON=0 / FDCM_POISON=1 python tools/refine_probe.py   the workspace filled with the word before every call

The digests must be equal (tests/test_gpu_refine.py runs the others in fresh processes, one after another: the switches are
read once per process)."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WINDOWS = ((None, 0, 0, 1, 1), (3, 1, 1, 1, 1), (2, 0, 2, 1, 3), (3, 2, 9, 1, 1))   # (na or None, hx, hy, sx, sy)


def case():
    """(scene, adopted (keys, volume, translation), templates, records per map)"""
    from openfdcm_amd import _capi, synthetic
    rng = np.random.default_rng(523)
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
        r["score"] = np.round(rng.uniform(0, 30, size=n))
        r["transform"] = np.stack([np.cos(a), -np.sin(a), rng.uniform(0, W, size=n), np.sin(a), np.cos(a), rng.uniform(0, H, size=n)], axis=1)
        r["transform"][::37, 1] = np.nan
        r[5::50] = r[4:-1:50]                                           # duplicates
        return r
    return synthetic.scene(90, 24, 11), (keys, vol, np.float32([3.5, -2.25])), tmpls, records


def run():
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    scene, (keys, vol, tr), tmpls, records = case()
    maps = [DeviceFeatureMap.build(scene, depth=12, coeff=5.0, padding=1.3, distance=0), DeviceFeatureMap.from_volume(keys, vol, tr)]
    pivots = np.array([[12.0, 12.0]] * len(tmpls), dtype=np.float32)
    h = hashlib.sha256()
    winners = moved = 0
    for dev in maps:
        recs = records(dev.width, dev.height, 600)
        for caps in (None, 2.0):
            tset = DeviceTemplates(tmpls, line_caps=caps)
            for q, (na, hx, hy, sx, sy) in enumerate(WINDOWS):
                cs = None
                if na is not None:
                    a = (np.arange(na) - na // 2) * np.deg2rad(2.0)
                    cs = np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)
                out, pose = dev.refine_matches(tset, recs, cs=cs, pivots=pivots if q % 2 else None, hx=hx, hy=hy, sx=sx, sy=sy, poses=True)
                for part in (out["score"], out["transform"]):
                    h.update(np.where(np.isnan(part), np.float32(np.nan), part).tobytes())
                h.update(out["tmpl_idx"].tobytes())
                h.update(pose.tobytes())
                won = pose[:, 0] >= 0
                winners += int(won.sum())
                moved += int((won & np.any(pose[:, 1:] != 0, axis=1)).sum())
    return h.hexdigest(), winners, moved


if __name__ == "__main__":
    digest, winners, moved = run()
    print(f"refine_probe {digest} winners {winners} moved {moved}")
