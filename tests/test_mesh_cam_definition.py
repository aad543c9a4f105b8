"""The referee of the pinhole mesh templates (tests/mesh_cam_ref.py) held to statements that do not come from it (include/fdcm.h,
"Templates from a mesh: pinhole views"): the lines of a cube one draws by hand, the outline of a sphere, the visibility of a
convex solid's contour, the orthographic limit, and record_camera_poses against a float64 projection.  CPU only: no call here reaches
the library's device code."""
import numpy as np
import pytest

import mesh_cam_cases as CC
import mesh_cam_ref as CR
import mesh_cases as MC
import mesh_join_ref as JR
import mesh_ref as MR


def _segments(lines):
    """The lines as a sorted list of end-point pairs, each pair ordered: what a drawing is, whatever the direction and order."""
    out = []
    for x0, y0, x1, y1 in np.asarray(lines, dtype=np.float64).reshape(-1, 4):
        a, b = (x0, y0), (x1, y1)
        out.append((a, b) if a <= b else (b, a))
    return sorted(out)


def _hand(v, edges, t, focal):
    """f x / d - O of the named cube edges in float64."""
    t = np.asarray(t, dtype=np.float64)
    P = v.astype(np.float64) + t
    d = -P[:, 2]
    pix = focal * P[:, :2] / d[:, None] - focal * t[:2] / -t[2]
    return _segments([(*pix[a], *pix[b]) for a, b in edges])


def _cube_vertex(x, y, z):
    return (x > 0) * 1 + (y > 0) * 2 + (z > 0) * 4        # mesh_cases.box_mesh: bit k of the index chooses hi on axis k


@pytest.mark.parametrize("visibility", ["items", "exact"])
@pytest.mark.parametrize("t,n_lines", [((3.0, 0.0, -6.0), 7), ((0.0, 0.0, -6.0), 4)])
def test_cube_lines_are_the_hand_drawing(t, n_lines, visibility):
    """The unit cube, R = 1, focal 240.  On the axis only the front face (z = +0.5) shows: 4 lines.  With the cube 3 to the right
    of the axis the camera also sees its side x = -0.5: the far vertical edge and the two edges that run back to it, 7 lines.
    Front face from -10.91 to 32.73 in X, the side face's far edge at -27.69."""
    v, f = MC.cube()
    mesh = MR.Mesh(v, f, MC.COS30)
    lines = CR.view_lines(mesh, MC.IDENTITY, t, 240.0, CR.default_near(v), MR.default_depth_tol(v), 2.0, visibility)
    V = _cube_vertex
    edges = [(V(-1, -1, 1), V(1, -1, 1)), (V(1, -1, 1), V(1, 1, 1)), (V(1, 1, 1), V(-1, 1, 1)), (V(-1, 1, 1), V(-1, -1, 1))]
    if n_lines == 7:
        edges += [(V(-1, -1, -1), V(-1, 1, -1)), (V(-1, -1, -1), V(-1, -1, 1)), (V(-1, 1, -1), V(-1, 1, 1))]
    want = _hand(v, edges, t, 240.0)
    got = _segments(lines)
    assert len(got) == n_lines == len(want)
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-3
    if n_lines == 7:
        xs = sorted({round(p[0], 2) for s in want for p in s})
        assert xs == [-27.69, -10.91, 32.73]


def _sphere_radius_at(alpha, D, focal):
    """The image radius of the unit sphere's point at polar angle alpha from the axis towards the camera at distance D."""
    return focal * np.sin(alpha) / (D - np.cos(alpha))


def test_icosphere_outline_is_the_tangent_cone():
    """The unit icosphere of 162 vertices at distance D = 3, focal 48: the outline circle has radius f r / sqrt(D^2 - r^2) =
    16.9706, not f r / D = 16.  No sphere point projects outside it, so no end point may, beyond rounding (1e-3 px).  From
    inside, the bound is the chord sag of the contour on the sphere: a contour edge lies between a face turned to the camera
    and one turned away, whose circumcentres lie on either side of the tangent circle (up to (1 - cos rho) / D, which the
    bound below swallows), so an end point is no further from the tangent circle, in angle on the sphere, than a face's
    circumradius rho -- which is below the longest edge's angle theta for these near-equilateral faces.  The image radius
    at polar angle alpha is f sin(alpha) / (D - cos(alpha)); the end points lie between its values at alpha_t +- theta and
    the outline radius."""
    v, f = MC.icosphere(2)
    assert len(v) == 162
    mesh = MR.Mesh(v, f, MC.COS30)
    assert mesh.sharp.sum() == 0
    D, focal = 3.0, 48.0
    R_out = focal / np.sqrt(D * D - 1.0)
    assert abs(R_out - 16.9706) < 1e-4
    v64 = v.astype(np.float64)
    theta = max(np.arccos(np.clip(v64[a] @ v64[b], -1, 1)) for a, b in mesh.everts)
    alpha_t = np.arccos(1.0 / D)
    low = min(_sphere_radius_at(alpha_t - theta, D, focal), _sphere_radius_at(alpha_t + theta, D, focal))
    for R in (MC.IDENTITY, MC.GENERIC):
        lines = CR.view_lines(mesh, R, (0.0, 0.0, -D), focal, CR.default_near(v), MR.default_depth_tol(v), 0.0, "exact")
        rad = np.hypot(lines[:, [0, 2]].astype(np.float64), lines[:, [1, 3]].astype(np.float64))
        print("icosphere outline: lines", len(lines), "radius", rad.min(), "..", rad.max(), "bounds", low, R_out)
        assert len(lines) >= 20
        assert rad.max() <= R_out + 1e-3 and rad.min() >= low - 1e-3
        assert rad.max() > 16.5        # (an orthographic outline would end at 16)


@pytest.mark.parametrize("name", ["cube", "tetrahedron", "icosphere"])
def test_contour_of_a_convex_solid_is_visible_under_exact_visibility(name):
    """A contour edge of a convex solid is on its silhouette: nothing is in front of it, so every sample of every such edge is
    visible under the exact rule.  (crease_cos = -1 leaves no sharp edge, so the candidates are the contours alone.)"""
    v, f, views, pos, focal = CC.case(name)
    mesh = MR.Mesh(v, f, -1.0)
    assert mesh.sharp.sum() == 0
    for R, t in zip(views, pos):
        runs, box, D, (X, Y, Z), seen = CR.view_runs(mesh, R, t, focal, CR.default_near(v), MR.default_depth_tol(v), "exact", want=True)
        assert len(seen) >= 3 and all(vis.all() for vis in seen.values()), name
        assert len(runs) == len(seen)


@pytest.mark.parametrize("name", CC.NAMES)
def test_cases_give_lines_and_fit_their_boxes(name):
    """Every case gives at least one line per view on the referee alone, in every mode the GPU tests compare; every box is
    under 300 pixels; the positions are at 3 to 8 diagonals."""
    v, f, views, pos, focal = CC.case(name)
    g = CC.diagonal(v)
    assert all(3.0 - 1e-6 <= -t[2] / g <= 8.0 + 1e-6 for t in pos)
    for R, t in zip(views, pos):
        X, Y, Z, d = CR.project(v, R, t, focal)
        box = MR.view_box(X, Y)
        assert CR.admitted(d, CR.default_near(v)) and box is not None
        assert box[2] - box[0] + 1 < CC.MAX_BOX and box[3] - box[1] + 1 < CC.MAX_BOX, box
    for visibility in ("items", "exact"):
        for tol in (None, 0.5):
            lines, off = CC.ref_lines(name, visibility, tol, 2.0)
            assert np.all(np.diff(off) >= 1), (name, visibility, tol, off)


@pytest.mark.parametrize("name,view", [("cube", MC.GENERIC), ("cube", MC.GENERIC2), ("tetrahedron", MC.GENERIC2),
                                       ("occluded_cubes", MC.GENERIC), ("l_prism", MC.GENERIC2), ("icosphere", MC.GENERIC)])
def test_far_camera_is_the_orthographic_view(name, view):
    """t = (0, 0, -2^20), focal = scale * 2^20: the line count is the orthographic referee's and the end points agree within
    1e-2 px, under the exact rule.  At that distance float32 keeps a depth to 1/8 of a mesh unit (the spacing of floats at
    2^20), so only decisions that do not hang on less carry over.  The exact rule's do on these solids: it never asks a face
    about a vertex it names, and every other hidden sample lies behind its occluder by a good part of the solid.  The item
    buffer's rule does not: next to a corner it judges a sample by the third face of that corner, whose plane passes within
    the depth tolerance (1e-4 diagonals) of the sample, far below 1/8 -- there the first or last sample of an edge may fall,
    which moves an end point by a pixel, in the limit's float32 arithmetic, not in the rule."""
    v, f = CC.MESHES[name]()
    mesh = MR.Mesh(v, f, MC.COS30)
    scale, D = 20.0, 2.0 ** 20
    tol = MR.default_depth_tol(v)
    want = JR.view_lines(mesh, view, np.float32(scale), tol, 2.0, "exact")
    got = CR.view_lines(mesh, view, (0.0, 0.0, -D), scale * D, CR.default_near(v), tol, 2.0, "exact")
    assert len(got) == len(want) > 0, (name, len(got), len(want))
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 1e-2


def test_refused_views():
    v, f = MC.cube()
    X, Y, Z, d = CR.project(v, MC.IDENTITY, (0.0, 0.0, -0.4), 100.0)     # the front face behind the camera
    assert not CR.admitted(d, 1e-3)
    assert CR.view_lines(MR.Mesh(v, f, MC.COS30), MC.IDENTITY, (0.0, 0.0, -0.4), 100.0, 1e-3, 0.0, 2.0) is None
    X, Y, Z, d = CR.project(v, MC.IDENTITY, (0.0, 0.0, -0.5), 100.0)     # d = 0 on the front face: 1 / d is infinite
    assert not CR.admitted(d, 1e-3)
    assert CR.admitted(CR.project(v, MC.IDENTITY, (0.0, 0.0, -0.75), 100.0)[3], 0.25)
    assert not CR.admitted(CR.project(v, MC.IDENTITY, (0.0, 0.0, -0.75), 100.0)[3], 0.26)


def _project64(v, R, T, focal, principal):
    P = v.astype(np.float64) @ R.T + T
    return np.asarray(principal) + focal * P[:, :2] / -P[:, 2:3]


def test_record_camera_poses_and_view_positions():
    import openfdcm_amd as O
    v, f = MC.notched_prism()
    views = O.view_rotations(6).astype(np.float64)
    g = CC.diagonal(v)
    positions = np.array([[0.3 * k - 0.5, 0.2 * k, -(4.0 + k) * g / 4] for k in range(6)])
    focal, principal = 700.0, (320.0, 240.0)
    rec = np.zeros(3, dtype=O._capi.MATCH_DTYPE)
    ang = np.deg2rad([30.0, 0.0, -110.0])
    rec["tmpl_idx"] = [4, 0, 2]
    deltas = np.array([[0.0, 0.0], [0.0, 0.0], [37.5, -12.25]])
    for i in range(3):
        c, s = np.cos(ang[i]), np.sin(ang[i])
        tv = positions[rec["tmpl_idx"][i]]
        o = focal * tv[:2] / -tv[2]
        xy = np.array(principal) + np.array([[c, -s], [s, c]]) @ o + deltas[i]
        rec["transform"][i] = [c, -s, xy[0], s, c, xy[1]]
    R_obj, T_obj = O.record_camera_poses(rec, views, positions, focal, principal)
    assert R_obj.shape == (3, 3, 3) and T_obj.shape == (3, 3) and R_obj.dtype == T_obj.dtype == np.float64
    assert np.array_equal(R_obj, O.record_rotations(rec, views)[0])
    for i in range(3):
        tr = rec["transform"][i].astype(np.float64)
        k = rec["tmpl_idx"][i]
        # the template's points in float64: the pinhole projection less the origin's
        origin_v = focal * positions[k][:2] / -positions[k][2]
        tmpl = _project64(v, views[k], positions[k], focal, (0.0, 0.0)) - origin_v
        rz2 = np.array([[tr[0], tr[1]], [tr[3], tr[4]]])
        moved = tmpl @ rz2.T + [tr[2], tr[5]]
        got = _project64(v, R_obj[i], T_obj[i], focal, principal)
        origin = _project64(np.zeros((1, 3)), R_obj[i], T_obj[i], focal, principal)[0]
        assert np.abs(origin - [tr[2], tr[5]]).max() <= 1e-9          # for any delta
        if deltas[i].any():
            # first order: a point at depth d moves by delta d0 / d, not delta
            d = -(v.astype(np.float64) @ R_obj[i].T + T_obj[i])[:, 2]
            d0 = -positions[k][2]
            err = np.hypot(*(got - moved).T)
            assert np.abs(err - np.hypot(*deltas[i]) * np.abs(d0 - d) / d).max() <= 1e-4 and err.max() > 1.0
        # delta = 0 exactly: the principal point that the record's own float32 (c, s, x, y) put there
        p0 = np.array([tr[2], tr[5]]) - rz2 @ origin_v
        R1, T1 = O.record_camera_poses(rec[i:i + 1], views, positions, focal, p0)
        assert np.abs(_project64(v, R1[0], T1[0], focal, p0) - moved).max() <= 1e-9, i
    assert np.array_equal(O.record_camera_poses(O.MatchList(rec), views, positions, focal, principal)[1], T_obj)
    with pytest.raises(ValueError):
        O.record_camera_poses(rec, views[:4], positions[:4], focal)
    with pytest.raises(ValueError):
        O.record_camera_poses(rec, views, positions[:5], focal)
    R0, T0 = O.record_camera_poses(rec[:0], views, positions, focal)
    assert R0.shape == (0, 3, 3) and T0.shape == (0, 3)
    # one position for all views; the default principal point
    one = O.record_camera_poses(rec, views, positions[0], focal)[1]
    assert one.shape == (3, 3)
    t = O.view_positions(5, 2.5)
    assert t.shape == (5, 3) and t.dtype == np.float32 and np.array_equal(t, np.tile(np.float32([0, 0, -2.5]), (5, 1)))
    for bad in ((0, 1.0), (3, 0.0), (3, float("nan"))):
        with pytest.raises(ValueError):
            O.view_positions(*bad)


def test_python_arguments_without_a_device():
    """Exactly one of scale and focal; positions' shape; the pinhole keywords without focal: all ValueError before any call of
    the library."""
    import openfdcm_amd as O
    mesh = O.Mesh(*MC.cube())
    for fn in (O.templates_from_mesh, O.mesh_view_lines):
        with pytest.raises(ValueError, match="exactly one"):
            fn(mesh, MC.IDENTITY)
        with pytest.raises(ValueError, match="exactly one"):
            fn(mesh, MC.IDENTITY, 10.0, focal=100.0, positions=(0, 0, -5))
        with pytest.raises(ValueError, match="positions"):
            fn(mesh, MC.IDENTITY, focal=100.0)
        with pytest.raises(ValueError, match="positions"):
            fn(mesh, np.stack([MC.IDENTITY] * 3), focal=100.0, positions=np.zeros((2, 3)))
        with pytest.raises(ValueError, match="pinhole"):
            fn(mesh, MC.IDENTITY, 10.0, positions=(0, 0, -5))
    with pytest.raises(ValueError, match="exactly one"):
        O.mesh_view_items(mesh, MC.IDENTITY)
    assert mesh.default_near() == CR.default_near(mesh.vertices) == np.float32(1e-3 * np.sqrt(3.0))
