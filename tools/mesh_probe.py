"""One fixed set of mesh-template calls (include/fdcm.h, "Templates from a mesh"), for comparing the library's paths: prints the
SHA-256 of the line records and offsets of 65 views of the L-prism and 9 views of the icosphere of tests/mesh_cases.py.

    python tools/mesh_probe.py                             the default path: every view in one part
    FDCM_MESH_PART=7 python tools/mesh_probe.py            parts of 7 views at most
    FDCM_POISON=0 / FDCM_POISON=1 python tools/mesh_probe.py   the scratch filled with the word as it is allocated

The digests must be equal (tests/test_gpu_mesh.py runs the others in fresh processes, one after another: the switches are read
once per process)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CALLS = (("l_prism", 65, 20.3, 0.0), ("icosphere", 9, 16.0, 2.0))   # mesh, views, scale, min_length


def run():
    import mesh_cases as MC
    from openfdcm_amd import engine
    h = hashlib.sha256()
    n_lines = 0
    for name, n, scale, min_length in CALLS:
        v, f = MC.MESHES[name]()
        mesh = engine.Mesh(v, f)
        rec, offsets = engine.mesh_view_lines(mesh, engine.view_rotations(n, hemisphere=False), scale, None, min_length)
        h.update(rec.tobytes())
        h.update(offsets.tobytes())
        n_lines += len(rec)
    return h.hexdigest(), n_lines


if __name__ == "__main__":
    digest, n_lines = run()
    print(f"mesh_probe {digest} lines {n_lines}")
