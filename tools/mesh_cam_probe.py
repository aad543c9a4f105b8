"""One fixed set of pinhole mesh-template calls (include/fdcm.h, "Templates from a mesh: pinhole views"), for comparing the
library's paths: prints the SHA-256 of the line records and offsets of 9 views of the L-prism, 9 of the icosphere and 5 of the
bumped icosphere of 1920 edges of tests/mesh_cases.py, each in the four modes {items, exact} x {no joining, 0.5}, the views at 3 to
6 diagonals of the mesh's bounding box and alternately on and off the camera's axis.

    python tools/mesh_cam_probe.py                            the default path: every view in one part
    FDCM_MESH_PART=2 python tools/mesh_cam_probe.py           parts of 2 views, writing runs of 32 lines
    FDCM_POISON=1 python tools/mesh_cam_probe.py              the scratch filled with the word as it is allocated

The digests must be equal (tests/test_gpu_mesh_cam.py runs the others in fresh processes, one after another: the switches are
read once per process)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CALLS = (("l_prism", 9, 800.0, 0.0), ("icosphere", 9, 500.0, 2.0), ("icosphere3_bumped", 5, 1000.0, 2.0))   # mesh, views, focal, min_length
MODES = (("items", None), ("items", 0.5), ("exact", None), ("exact", 0.5))


def positions(n, diagonal):
    """View k at 3 + 3 k / n diagonals; every other view 0.4 diagonals off the axis, in a direction that turns with k."""
    k = np.arange(n, dtype=np.float64)
    off = np.where(k % 2 == 1, 0.4, 0.0)
    return (np.stack([off * np.cos(k), off * np.sin(k), -(3.0 + 3.0 * k / n)], axis=1) * diagonal).astype(np.float32)


def results():
    """(line records, offsets) of every call in every mode, call after call."""
    import mesh_cases as MC
    from openfdcm_amd import engine
    out = []
    for name, n, focal, min_length in CALLS:
        v, f = MC.MESHES[name]()
        d = v.astype(np.float64).max(axis=0) - v.astype(np.float64).min(axis=0)
        mesh, views = engine.Mesh(v, f), engine.view_rotations(n, hemisphere=False)
        t = positions(n, float(np.sqrt(d @ d)))
        out += [engine.mesh_view_lines(mesh, views, None, None, min_length, vis, tol, focal=focal, positions=t) for vis, tol in MODES]
    return out


def digest(results):
    h = hashlib.sha256()
    for rec, offsets in results:
        h.update(rec.tobytes())
        h.update(offsets.tobytes())
    return h.hexdigest(), sum(len(rec) for rec, _ in results)


if __name__ == "__main__":
    d, n_lines = digest(results())
    print(f"mesh_cam_probe {d} lines {n_lines}")
