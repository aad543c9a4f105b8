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


# ---------------------------------------------------------------------------------------------------------------------------
# What the shapes of tests/test_gpu_mesh.py reach, stated on the referee alone: a GPU comparison that no longer ran a kernel's
# second pass, second block or late write would stay green, so each condition is counted here from the header's rules.

def _rotations(n):
    from openfdcm_amd.engine import view_rotations     # pure numpy
    return view_rotations(n, hemisphere=False)


def test_forty_views_of_the_cubes_list_432_faces():
    """The header's tile rule: a face of non-zero area whose pixel box takes more than 64 tiles of 4 x 4 goes onto the list; 16
    slices per listed face on a grid of 2048 workgroups."""
    v, f = MC.occluded_cubes()
    listed = 0
    for R in _rotations(40):
        X, Y, _ = MR.project(v, R, np.float32(40.0))
        for A, B, C in f.tolist():
            xs, ys = np.floor(X[[A, B, C]]).astype(np.int64), np.floor(Y[[A, B, C]]).astype(np.int64)
            tiles = (((int(xs.max()) - int(xs.min())) >> 2) + 1) * (((int(ys.max()) - int(ys.min())) >> 2) + 1)
            a = MR._orient(X[A], Y[A], X[B], Y[B], X[C], Y[C])
            listed += bool(tiles > 64 and (a > 0 or a < 0))
    assert listed == 432 and listed > 128 and 16 * listed == 6912 > 3 * 2048
    lines, offsets = MR.views_lines(MR.Mesh(v, f, MC.COS30), _rotations(40), np.float32(40.0), MR.default_depth_tol(v), 2.0)
    assert len(lines) == 688 and len(offsets) == 41


def test_three_hundred_views_carry_into_the_second_256_sums():
    v, f = MC.tetrahedron()
    mesh = MR.Mesh(v, f, MC.COS30)
    nb = 300 * ((len(mesh.everts) + 255) // 256)
    assert nb == 300 > 256
    lines, offsets = MR.views_lines(mesh, _rotations(300), np.float32(9.3), MR.default_depth_tol(v), 0.0)
    per_view = np.diff(offsets)
    assert len(lines) == 1553 and per_view.min() == 3 and per_view.max() == 9
    assert offsets[256] == 1321 > 0
    bad = np.diag([5000.0, 1.0, 1.0]).astype(np.float32)
    assert MR.view_box(*MR.project(v, bad, np.float32(9.3))[:2]) is None


def test_bumped_icosphere_fills_every_block():
    v, f, views, scale = MC.case("icosphere3_bumped")
    mesh = MR.Mesh(v, f, MC.COS30)
    E = len(mesh.everts)
    assert (len(v), len(f), E, int(mesh.sharp.sum())) == (642, 1280, 1920, 80)
    nbV, nbE = (len(v) + 255) // 256, (E + 255) // 256
    assert nbV == 3 and nbE == 8 and (len(f) + 15) // 16 == 80
    tol = MR.default_depth_tol(v)
    totals, late = [], 0
    for R in views:
        X, Y, Z = MR.project(mesh.v, R, scale)
        box = MR.view_box(X, Y)
        D = MR.item_buffer(mesh, X, Y, Z, box)
        per_block = np.zeros(nbE, dtype=np.int64)
        for e in np.nonzero(MR.candidates(mesh, X, Y))[0]:
            per_block[e // 256] += len(MR.edge_lines(mesh, X, Y, Z, box, D, e, tol, 0.0)[0])
        assert per_block.min() >= 3, per_block      # every edge block of every view writes lines
        totals.append(int(per_block.sum()))
        # a side of the box that only vertices of the second and third blocks reach: the first block's atomics alone get it wrong
        fx, fy = np.floor(X), np.floor(Y)
        sides = [np.nonzero(c)[0] for c in (fx == fx.min(), fx == fx.max(), fy == fy.min(), fy == fy.max())]
        late += any(s.min() >= 256 for s in sides)
        if R is views[0]:
            assert [int(i) for i in (np.argmin(X), np.argmax(X), np.argmin(Y), np.argmax(Y))] == [275, 148, 498, 14]
        if R is views[1]:
            assert [int(i) for i in (np.argmin(X), np.argmax(X), np.argmin(Y), np.argmax(Y))] == [283, 40, 147, 256]
    assert totals[:2] == [94, 123] and late >= 2
    # the probe's five views: each more than the 32 lines of a forced writing run, so each starts a run of its own
    _, offsets = MR.views_lines(mesh, _rotations(5), scale, tol, 0.0)
    assert np.diff(offsets).min() > 32


def _fence_edge_runs(view, scale, min_length, pair):
    v, f = MC.fence()
    mesh = MR.Mesh(v, f, MC.COS30)
    X, Y, Z = MR.project(mesh.v, view, np.float32(scale))
    box = MR.view_box(X, Y)
    D = MR.item_buffer(mesh, X, Y, Z, box)
    e = [i for i, p in enumerate(mesh.everts.tolist()) if p == list(pair)][0]
    assert MR.candidates(mesh, X, Y)[e]
    total = len(MR.view_lines(mesh, view, np.float32(scale), MR.default_depth_tol(v), min_length))
    return np.array(MR.edge_lines(mesh, X, Y, Z, box, D, e, MR.default_depth_tol(v), min_length)[0], dtype=np.float64), box, total


def test_fence_edges_carry_41_lines():
    for view, scale in ((MC.IDENTITY, 8.0), (MC.FENCE_TURNED, 7.3)):
        for min_length in (0.0, 2.0):
            for pair in ((0, 1), (2, 3)):
                runs, box, total = _fence_edge_runs(view, scale, min_length, pair)
                assert len(runs) == 41, (scale, min_length, pair, len(runs))
                assert total == 244      # 2 x 41, and 4 of each of the 40 slats, 2 of the sheet's ends
                assert box[2] - box[0] + 1 == 969 or scale != 8.0


def test_fence_runs_are_the_gaps_between_the_slats():
    """Edge (0, 1) under the identity at 8 px per unit is y = 0 from x = 0 to 968; slat k hides x in (24 k + 10, 24 k + 22)."""
    K, s = 40, 8.0
    runs, _, _ = _fence_edge_runs(MC.IDENTITY, s, 0.0, (0, 1))
    assert runs.shape == (41, 4) and np.all(runs[:, [1, 3]] == 0.0)
    slats = [(s * (3 * k + 1.25), s * (3 * k + 2.75)) for k in range(K)]
    outline = np.array([0.0, s * (3 * K + 1)] + [x for sl in slats for x in sl])
    for x in np.concatenate([runs[:, 0], runs[:, 2]]):
        assert np.abs(outline - x).min() <= 1.5, x
    for xa, xb in np.sort(runs[:, [0, 2]], axis=1).tolist():
        for lo, hi in slats:
            assert min(xb, hi) - max(xa, lo) <= 1.5, (xa, xb, lo, hi)
    # and each gap has its run: run k from the end of slat k - 1 to the start of slat k, in k0 order
    for k, (xa, xb) in enumerate(runs[:, [0, 2]].tolist()):
        assert abs(xa - (0.0 if k == 0 else slats[k - 1][1])) <= 1.5 and abs(xb - (s * (3 * K + 1) if k == K else slats[k][0])) <= 1.5, (k, xa, xb)


def test_cube_at_4095_is_the_square_of_4096_pixels():
    """The largest view the call takes: an item buffer of 4096 x 4096 keys, 128 MB, so five of them exceed a part's 512 MB and
    three do not.  The lines, in the referee's order (tests/test_gpu_mesh.py holds the device to these four)."""
    v, f = MC.cube()
    mesh = MR.Mesh(v, f, MC.COS30)
    lines, box, D = MR.view_lines(mesh, MC.IDENTITY, np.float32(4095.0), MR.default_depth_tol(v), 2.0, want_items=True)
    assert box == (-2048, -2048, 2047, 2047) and D.shape == (4096, 4096) and D.nbytes == 128 << 20
    h = 2047.5
    want = [[-h, -h, h, -h], [-h, -h, -h, h], [h, -h, h, h], [-h, h, h, h]]
    assert lines.tobytes() == np.array(want, dtype=np.float32).tobytes()


def test_tall_triangles_sit_on_either_side_of_64_tiles():
    v, f, views, scale = MC.case("triangle-3x257")
    for R, rows in zip(views, (257, 256)):
        X, Y, _ = MR.project(v, R, scale)
        box = MR.view_box(X, Y)
        tx, ty = ((box[2] - box[0]) >> 2) + 1, ((box[3] - box[1]) >> 2) + 1
        assert (box[2] - box[0] + 1, box[3] - box[1] + 1) == (3, rows) and tx == 1 and (ty > 64) == (rows == 257)
