"""One fixed set of calls on match lists with objects and hull shapes (include/fdcm.h, "Match lists: objects and hull shapes"),
for comparing the library's paths: prints the SHA-256 of the device's span tables and of the records, positions, boxes and
matched fractions of fdcm_matches_detect_objects on box and hull sets.

    python tools/match_objects_probe.py                            the default path
    FDCM_MATCHED_FLAT=1 python tools/match_objects_probe.py        64-bit flat addresses
    FDCM_FORCE_HOST_BINS=1 python tools/match_objects_probe.py     the bins from the host libm
    FDCM_POISON=0 / FDCM_POISON=1 python tools/match_objects_probe.py   the workspace and the span table filled with the word

The digests must be equal (tests/test_gpu_match_objects.py runs the others in fresh processes, one after another: the switches
are read once per process)."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_probe  # noqa: E402  (the case: two maps, templates of 0 to 130 lines, 600 records of every kind)


def run():
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    scene, (keys, vol, tr), tmpls, records = match_probe.case()
    maps = [DeviceFeatureMap.build(scene, depth=12, coeff=5.0, padding=1.3, distance=0), DeviceFeatureMap.from_volume(keys, vol, tr)]
    objects = np.arange(len(tmpls), dtype=np.int32) % 3
    h = hashlib.sha256()
    rows = kept = 0
    for dev in maps:
        recs = records(dev.width, dev.height, 600)
        for margin in (0, 2):
            off, spans, areas = dev.match_shapes(DeviceTemplates(tmpls), recs, margin=margin)
            for part in (off, spans, areas):
                h.update(part.tobytes())
            rows += int(off[-1])
        for kind in ("box", "hull"):
            for caps in (None, 2.0):
                tset = DeviceTemplates(tmpls, line_caps=caps, footprint=kind)
                for kw in (dict(penalty=0, overlap_permille=300, cross_permille=800), dict(overlap_permille=0, cross_permille=0, max_detections=200, rescore=True),
                           dict(penalty=0, overlap_permille=150, cross_permille=1000, min_matched=[0.4, 0.0, 0.2], max_score=[6.0, 9.0, 4.0], margin=2,
                                rescore=True)):
                    kw = {"max_score": np.inf, **kw}
                    res = dev.detect_matches_objects(tset, recs, objects, indices=True, boxes=True, matched=True, **kw)
                    for part in res:
                        h.update(part.tobytes())
                    kept += len(res[0])
    return h.hexdigest(), rows, kept


if __name__ == "__main__":
    digest, rows, kept = run()
    print(f"match_objects_probe {digest} rows {rows} kept {kept}")
