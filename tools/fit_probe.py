"""One fixed set of pose-fit calls on match records (include/fdcm.h, "Match lists: pose fit"), for comparing the library's
paths: prints the SHA-256 of the fitted records, the info rows and the rms values, on the 300 records of tests/fit_cases.py's
world "b5-d6" at three of its parameter sets.

    python tools/fit_probe.py [n]                        the default path, on the first n records (300)
    FDCM_FORCE_HOST_BINS=1 python tools/fit_probe.py     the bins from the host libm, downloaded records every pass
    FDCM_COVERAGE_PART=90 python tools/fit_probe.py      the list in parts of 90 records
    FDCM_POISON=0 / FDCM_POISON=1 python tools/fit_probe.py   the coverage buffers filled with the word before every call

The digests must be equal (tests/test_gpu_fit.py runs the others in fresh processes, one after another: the switches are read
once per process)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WORLD, PARAMS = "b5-d6", (1, 2, 4)   # fit_cases.PARAMS[k]: radius 1, m / 2, 8 steps; radius 32, 8 steps; radius 3 without damping


def run(n=300):
    import fit_cases as FC
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    w = FC.world(WORLD)
    dev = DeviceFeatureMap.build_labels(w.labels, border=w.border, depth=w.depth)
    tset = DeviceTemplates(w.tmpls)
    h = hashlib.sha256()
    stepped = stopped = 0
    for k in PARAMS:
        out, info, rms = dev.fit_matches(w.labels, tset, w.recs[:n], tmpl_index_base=w.base, info=True, rms=True, **w.kw(*FC.PARAMS[k]))
        for part in (out, info, rms):
            h.update(part.tobytes())
        stepped += int((info[:, 1] > 0).sum())
        stopped += int((info[:, 0] > 0).sum())
    return h.hexdigest(), stepped, stopped


if __name__ == "__main__":
    digest, stepped, stopped = run(int(sys.argv[1]) if len(sys.argv) > 1 else 300)
    print(f"fit_probe {digest} stepped {stepped} stopped {stopped}")
