"""One fixed set of mesh-template calls (include/fdcm.h, "Templates from a mesh"), for comparing the library's paths: prints the
SHA-256 of the line records and offsets of 65 views of the L-prism, 9 views of the icosphere and 5 views of the bumped icosphere
of 1920 edges (8 edge blocks a view) of tests/mesh_cases.py.

    python tools/mesh_probe.py                             the default path: every view in one part
    FDCM_MESH_PART=7 python tools/mesh_probe.py            parts of 7 views at most
    FDCM_MESH_PART=2 python tools/mesh_probe.py            parts of 2, and writing runs of 32 lines: a run per view of the third call
    FDCM_POISON=0 / FDCM_POISON=1 python tools/mesh_probe.py   the scratch filled with the word as it is allocated

The digests must be equal (tests/test_gpu_mesh.py runs the others in fresh processes, one after another: the switches are read
once per process)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CALLS = (("l_prism", 65, 20.3, 0.0), ("icosphere", 9, 16.0, 2.0), ("icosphere3_bumped", 5, 33.7, 0.0))   # mesh, views, scale, min_length


def results():
    """(line records, offsets) of every call."""
    import mesh_cases as MC
    from openfdcm_amd import engine
    out = []
    for name, n, scale, min_length in CALLS:
        v, f = MC.MESHES[name]()
        out.append(engine.mesh_view_lines(engine.Mesh(v, f), engine.view_rotations(n, hemisphere=False), scale, None, min_length))
    return out


def digest(results):
    h = hashlib.sha256()
    for rec, offsets in results:
        h.update(rec.tobytes())
        h.update(offsets.tobytes())
    return h.hexdigest(), sum(len(rec) for rec, _ in results)


def run():
    return digest(results())


if __name__ == "__main__":
    digest, n_lines = run()
    print(f"mesh_probe {digest} lines {n_lines}")
