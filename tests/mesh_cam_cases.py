"""The cases of the pinhole mesh-template tests (include/fdcm.h, "Templates from a mesh: pinhole views"): meshes of
tests/mesh_cases.py seen by a pinhole camera, on and off its axis, at 3 to 8 diagonals of the mesh's bounding box, with focal
lengths that keep every view's pixel box under 300 pixels.  The bumped icosphere has 3 vertex and 8 edge blocks a view, so the
grid splits run; the fence has 41 runs on an edge; the occluded cubes and the prisms have edges cut by faces in front of them,
which under perspective are cut elsewhere than in the orthographic view.  The referee's runs per (case, visibility) are computed
once and shared (they depend on neither min_length nor the joining)."""
import numpy as np

import mesh_cam_ref as CR
import mesh_cases as MC
import mesh_ref as MR

MESHES = dict(MC.MESHES, notched_prism=MC.notched_prism)
MAX_BOX = 300


def diagonal(v):
    d = v.astype(np.float64).max(axis=0) - v.astype(np.float64).min(axis=0)
    return float(np.sqrt(d @ d))


# (name, mesh, views, positions in bounding-box diagonals, focal)
CASES = [
    ("cube", "cube", [MC.IDENTITY, MC.GENERIC, MC.GENERIC2], [(0, 0, -3), (0.9, -0.4, -4), (-1.5, 1.0, -8)], 640.0),
    ("tetrahedron", "tetrahedron", [MC.IDENTITY, MC.GENERIC], [(0.5, 0.3, -3), (0, 0, -5)], 700.0),
    ("l_prism", "l_prism", [MC.IDENTITY, MC.GENERIC2, MC.SIDE], [(0, 0, -3), (-1.0, 0.5, -4), (0.3, 0.3, -6)], 800.0),
    ("notched_prism", "notched_prism", [MC.GENERIC, MC.GENERIC2], [(0, 0, -5), (1.0, -1.0, -3.5)], 900.0),
    ("occluded_cubes", "occluded_cubes", [MC.IDENTITY, MC.GENERIC], [(0, 0, -3), (0.6, 0.2, -4)], 700.0),
    ("fence", "fence", [MC.IDENTITY, MC.FENCE_TURNED], [(0, 0, -3), (0.2, 0.05, -4)], 600.0),
    ("icosphere", "icosphere", [MC.GENERIC, MC.GENERIC2], [(0, 0, -3), (0.7, 0.7, -5)], 500.0),
    ("icosphere3_bumped", "icosphere3_bumped", [MC.GENERIC, MC.IDENTITY], [(0, 0, -3), (-0.8, 0.5, -6)], 1000.0),
]
NAMES = [c[0] for c in CASES]


def case(name):
    """(vertices, faces, views (n, 3, 3), positions (n, 3) float32, focal float32)"""
    for n, mesh, views, pos, focal in CASES:
        if n == name:
            v, f = MESHES[mesh]()
            t = (np.asarray(pos, dtype=np.float64) * diagonal(v)).astype(np.float32)
            return v, f, np.stack(views), t, np.float32(focal)
    raise KeyError(name)


_mesh, _runs = {}, {}


def ref_mesh(name):
    if name not in _mesh:
        v, f = case(name)[:2]
        _mesh[name] = MR.Mesh(v, f, MC.COS30)
    return _mesh[name]


def ref_runs(name, visibility):
    """Per view of the case the referee's runs at the default tolerance and near."""
    key = (name, visibility)
    if key not in _runs:
        v, f, views, pos, focal = case(name)
        _runs[key] = [CR.view_runs(ref_mesh(name), R, t, focal, CR.default_near(v), MR.default_depth_tol(v), visibility)
                      for R, t in zip(views, pos)]
    return _runs[key]


def ref_lines(name, visibility, tol, min_length, only=None):
    """(lines (N, 4) float32, offsets) of the case's views (or of the views `only`) from the shared runs."""
    import mesh_join_ref as JR
    runs = ref_runs(name, visibility)
    parts = [JR.lines_of_runs(runs[i], min_length, tol) for i in (range(len(runs)) if only is None else only)]
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in parts], out=offsets[1:])
    return np.concatenate(parts).reshape(-1, 4), offsets


_raster = {}


def ref_raster(name):
    """Per view of the case the referee's pixel box and item buffer."""
    if name not in _raster:
        v, f, views, pos, focal = case(name)
        out = []
        for R, t in zip(views, pos):
            X, Y, Z, d = CR.project(ref_mesh(name).v, R, t, focal)
            assert CR.admitted(d, CR.default_near(v))
            box = MR.view_box(X, Y)
            out.append((box, MR.item_buffer(ref_mesh(name), X, Y, Z, box)))
        _raster[name] = out
    return _raster[name]
