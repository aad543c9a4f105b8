"""The referee of the mesh templates (tests/mesh_ref.py; include/fdcm.h, "Templates from a mesh") against geometry that does not
come from it: the visible edges of solids whose views can be drawn by hand.  No device, no library."""
import numpy as np

import mesh_cases as MC
import mesh_ref as MR

def _lines(name, view, scale, crease_cos=MC.COS30, depth_tol=None, min_length=2.0):
    v, f = MC.MESHES[name]()
    mesh = MR.Mesh(v, f, crease_cos)
    tol = MR.default_depth_tol(v) if depth_tol is None else depth_tol
    return mesh, MR.view_lines(mesh, view, np.float32(scale), tol, min_length)


def _undirected(lines, digits=3):
    out = set()
    for x1, y1, x2, y2 in np.round(lines.astype(np.float64), digits).tolist():
        out.add(tuple(sorted([(x1 + 0.0, y1 + 0.0), (x2 + 0.0, y2 + 0.0)])))
    return out


def _segment(p, q):
    return tuple(sorted([(float(p[0]), float(p[1])), (float(q[0]), float(q[1]))]))


def test_cube_along_an_axis_is_the_square():
    s = 65.0    # the outline runs through pixel centres: the top face covers every pixel a sample of the lower edges falls into
    _, lines = _lines("cube", MC.IDENTITY, s)
    h = s / 2
    c = [(-h, -h), (h, -h), (h, h), (-h, h)]
    assert lines.shape == (4, 4)
    assert _undirected(lines) == {_segment(c[i], c[(i + 1) % 4]) for i in range(4)}


def test_cube_from_a_generic_view_hides_the_far_corner():
    s = 65.0
    mesh, lines = _lines("cube", MC.GENERIC, s)
    X, Y, Z = MR.project(mesh.v, MC.GENERIC, np.float32(s))
    far = int(np.argmin(Z))
    want = set()
    for e, (a, b) in enumerate(mesh.everts.tolist()):
        if mesh.sharp[e] and far not in (a, b):
            want.add(_segment((X[a], Y[a]), (X[b], Y[b])))
    assert len(want) == 9 and int(mesh.sharp.sum()) == 12
    assert lines.shape == (9, 4) and _undirected(lines) == {tuple((round(x, 3) + 0.0, round(y, 3) + 0.0) for x, y in seg) for seg in want}


def test_open_square_is_its_boundary():
    s = 31.5
    mesh, lines = _lines("open_square", MC.GENERIC, s)
    X, Y, _ = MR.project(mesh.v, MC.GENERIC, np.float32(s))
    assert int(mesh.sharp.sum()) == 4 and len(mesh.everts) == 5
    want = {_segment((X[i], Y[i]), (X[(i + 1) % 4], Y[(i + 1) % 4])) for i in range(4)}
    assert _undirected(lines) == {tuple((round(x, 3) + 0.0, round(y, 3) + 0.0) for x, y in seg) for seg in want}


def test_icosphere_gives_contours_on_the_circle():
    s, r = 16.0, 1.0
    v, f = MC.icosphere()
    # the outline of an inscribed convex solid lies between the circle and the circle shrunk by the cosine of the covering
    # radius: the largest angle between a face's circumcentre direction and its vertices
    vv = v.astype(np.float64)
    nrm = np.cross(vv[f[:, 1]] - vv[f[:, 0]], vv[f[:, 2]] - vv[f[:, 0]])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    cosrho = np.abs(np.einsum("ij,ij->i", nrm, vv[f[:, 0]])).min()
    sag = s * r * (1.0 - cosrho)
    assert sag + 1e-3 < 1.0
    for view in (MC.IDENTITY, MC.GENERIC, MC.GENERIC2):
        mesh, lines = _lines("icosphere", view, s)
        assert int(mesh.sharp.sum()) == 0 and len(lines) >= 5
        rad = np.hypot(lines[:, [0, 2]].astype(np.float64), lines[:, [1, 3]].astype(np.float64))
        assert np.all(rad <= s * r + 1e-3) and np.all(rad >= s * r - 1.0), (rad.min(), rad.max())
        assert np.all(rad >= s * r - sag - 1e-3)
        # each contour edge at most once: together no longer than the circle.  (They need not close it: a sample whose pixel a
        # neighbouring face owns is held against that face's plane continued to the sample, which lies above a convex surface.)
        _, every = _lines("icosphere", view, s, min_length=0.0)
        total = np.hypot(every[:, 2] - every[:, 0], every[:, 3] - every[:, 1]).astype(np.float64).sum()
        assert total <= 2 * np.pi * s * r + 1e-2, total


def test_roof_ridge_is_one_line_at_the_grazing_view():
    s = 60.0
    mesh, lines = _lines("roof", MC.GRAZING, s)
    X, Y, _ = MR.project(mesh.v, MC.GRAZING, np.float32(s))
    ridge = _segment((X[0], Y[0]), (X[1], Y[1]))
    assert tuple((round(x, 3) + 0.0, round(y, 3) + 0.0) for x, y in ridge) in _undirected(lines)
    # the sibling triangle does take pixels under the ridge's samples, and its plane at the pixel centre would hide them
    _, box, D = MR.view_lines(mesh, MC.GRAZING, np.float32(s), MR.default_depth_tol(mesh.v), 2.0, want_items=True)
    e = [i for i, p in enumerate(mesh.everts.tolist()) if p == [0, 1]][0]
    Xs, Ys, Zs = MR.project(mesh.v, MC.GRAZING, np.float32(s))
    _, vis = MR.edge_lines(mesh, Xs, Ys, Zs, box, D, e, MR.default_depth_tol(mesh.v), 2.0)
    assert vis.all()
    n = len(vis) - 1
    owners = set()
    for k in range(n + 1):
        t = np.float32(k) / np.float32(n)
        px, py = int(np.floor(Xs[0] + t * (Xs[1] - Xs[0]))), int(np.floor(Ys[0] + t * (Ys[1] - Ys[0])))
        if box[0] <= px <= box[2] and box[1] <= py <= box[3] and D[py - box[1], px - box[0]]:
            owners.add(int(D[py - box[1], px - box[0]]) & 0xFFFFFFFF)
    assert owners - {int(mesh.efaces[e, 0]), int(mesh.efaces[e, 1])}, owners


def test_occluded_edges_end_at_the_occluders_outline():
    s = 40.0
    mesh, lines = _lines("occluded_cubes", MC.IDENTITY, s)
    on_edge = lines[(lines[:, 0] == s) & (lines[:, 2] == s)]    # the large cube's edges along x = 1
    assert len(on_edge) >= 2
    crossings = (-0.3 * s, 0.3 * s)
    ends = np.concatenate([on_edge[:, 1], on_edge[:, 3]]).astype(np.float64)
    for y in ends:
        assert min(abs(y - c) for c in crossings + (-s, s)) <= 2.5, y
    for c in crossings:
        assert np.min(np.abs(ends - c)) <= 2.5
    for _, y1, _, y2 in on_edge.astype(np.float64).tolist():    # nothing is drawn behind the small cube
        lo, hi = min(y1, y2), max(y1, y2)
        assert hi <= crossings[0] + 2.5 or lo >= crossings[1] - 2.5, (lo, hi)


def test_l_prism_concave_edge_and_degenerate_faces():
    mesh, lines = _lines("l_prism", MC.IDENTITY, 20.3)
    assert len(lines) >= 6
    v, f = MC.with_degenerate_faces()
    mesh = MR.Mesh(v, f, MC.COS30)
    e = [i for i, p in enumerate(mesh.everts.tolist()) if p == [8, 9]][0]
    assert mesh.efaces[e].tolist() == [12, 13] and mesh.sharp[e] == 1
    try:
        MR.Mesh(*MC.non_manifold(), MC.COS30)
        raise AssertionError("a third face on an edge was accepted")
    except MR.NonManifold:
        pass


def test_views_are_independent_and_ordered():
    v, f, views, scale = MC.case("tetrahedron")
    mesh = MR.Mesh(v, f, MC.COS30)
    lines, offsets = MR.views_lines(mesh, views, scale, MR.default_depth_tol(v), 0.0)
    assert offsets[0] == 0 and offsets[-1] == len(lines) and np.all(np.diff(offsets) > 0)
    for i, R in enumerate(views):
        assert MR.view_lines(mesh, R, scale, MR.default_depth_tol(v), 0.0).tobytes() == lines[offsets[i]:offsets[i + 1]].tobytes()
