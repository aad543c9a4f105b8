"""One fixed set of mesh-template calls with exact visibility and joined lines (include/fdcm.h, "Templates from a mesh: exact
visibility and joined lines"), for comparing the library's paths: prints the SHA-256 of the line records and offsets of 9 views
of the L-prism, 9 of the icosphere and 5 of the bumped icosphere of 1920 edges of tests/mesh_cases.py, each in the four modes
{items, exact} x {no joining, 0.5}.

    python tools/mesh_join_probe.py                            the default path: every view in one part
    FDCM_MESH_PART=2 python tools/mesh_join_probe.py           parts of 2 views, writing runs of 32 lines
    FDCM_POISON=1 python tools/mesh_join_probe.py              the scratch filled with the word as it is allocated

The digests must be equal (tests/test_gpu_mesh_join.py runs the others in fresh processes, one after another: the switches are
read once per process)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CALLS = (("l_prism", 9, 20.3, 0.0), ("icosphere", 9, 16.0, 2.0), ("icosphere3_bumped", 5, 33.7, 2.0))   # mesh, views, scale, min_length
MODES = (("items", None), ("items", 0.5), ("exact", None), ("exact", 0.5))


def results():
    """(line records, offsets) of every call in every mode, call after call."""
    import mesh_cases as MC
    from openfdcm_amd import engine
    out = []
    for name, n, scale, min_length in CALLS:
        v, f = MC.MESHES[name]()
        mesh, views = engine.Mesh(v, f), engine.view_rotations(n, hemisphere=False)
        out += [engine.mesh_view_lines(mesh, views, scale, None, min_length, vis, tol) for vis, tol in MODES]
    return out


def digest(results):
    h = hashlib.sha256()
    for rec, offsets in results:
        h.update(rec.tobytes())
        h.update(offsets.tobytes())
    return h.hexdigest(), sum(len(rec) for rec, _ in results)


if __name__ == "__main__":
    d, n_lines = digest(results())
    print(f"mesh_join_probe {d} lines {n_lines}")
