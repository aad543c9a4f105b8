"""One fixed set of calls with objects (include/fdcm.h, "Objects"), for comparing the library's paths: prints the SHA-256 of
the object best map's planes, of the dense records, boxes and fractions and of the windows' records, boxes, fractions and job
indices, all at FDCM_GATE_ALL with thresholds and needs per object.

    python tools/objects_probe.py --max-score <float.hex(),..>                      the default path
    FDCM_MATCHED_FLAT=1 python tools/objects_probe.py --max-score ..    64-bit flat addresses in the dense calls
    FDCM_WINDOWS_FLAT=1 python tools/objects_probe.py --max-score ..    .. in the pose windows

The digests must be equal (tests/test_gpu_objects.py runs the switches in fresh processes: they are read once per process).
The case is tools/gate_probe.py's with labels: five objects, of which object 3 is empty and object 4 holds only the template
without lines, and no object's templates are contiguous.  --max-score: one threshold per object, as float.hex(), from the
process that compares (a process under a switch must not derive its own); without it every threshold is +inf."""
import importlib.util
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OBJECTS = [4, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1]
G = 5
MIN_MATCHED = (0.0, 0.5, 0.3, 0.5, 0.0)
OVERLAP, CROSS = 300, 600


def gate_probe():
    spec = importlib.util.spec_from_file_location("gate_probe", os.path.join(os.path.dirname(os.path.abspath(__file__)), "gate_probe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def calls(dev, tset, cs, piv, job_list, max_score, gp=None):
    """The object best map and the dense call with rotations, and the windows' call, at FDCM_GATE_ALL: what the digest covers."""
    gp = gp or gate_probe()
    grid = dev.exhaustive_rotations_window(tset, cs, piv, *gp.STRIDE).as_tuple()
    planes = dev.best_map_objects(tset, grid, OBJECTS, G, cs, piv, penalty=0, min_matched=MIN_MATCHED, matched=True)
    dense = dev.exhaustive_detect_objects(tset, grid, OBJECTS, max_score, G, cs, piv, max_detections=4096, overlap_permille=OVERLAP,
                                          cross_permille=CROSS, margin=gp.MARGIN, penalty=0, min_matched=MIN_MATCHED, boxes=True,
                                          matched=True, gate="all")
    win = dev.exhaustive_detect_windows_objects(tset, job_list, OBJECTS, max_score, G, cs, piv, sx=gp.STRIDE[0], sy=gp.STRIDE[1],
                                                wrap=True, max_detections=4096, overlap_permille=OVERLAP, cross_permille=CROSS,
                                                margin=gp.MARGIN, penalty=0, min_matched=MIN_MATCHED, boxes=True, matched=True,
                                                job_index=True, gate="all")
    return planes, dense, win


def run(max_score):
    from openfdcm_amd.engine import DeviceTemplates
    gp = gate_probe()
    dev, tmpls, caps, cs, piv, job_list = gp.case()
    planes, dense, win = calls(dev, DeviceTemplates(tmpls, line_caps=caps), cs, piv, job_list, max_score, gp)
    return gp.digest(planes + dense + win), len(dense[0]) + len(win[0])


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--max-score", default=None, help="float.hex() of every object's threshold, separated by commas")
    a = ap.parse_args()
    ms = [float("inf")] * G if a.max_score is None else [float.fromhex(v) for v in a.max_score.split(",")]
    d, n = run(ms)
    print("objects_probe", d, "records", n)
