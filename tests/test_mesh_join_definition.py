"""The referee of the exact visibility and the joined lines of the mesh templates (tests/mesh_join_ref.py; include/fdcm.h,
"Templates from a mesh: exact visibility and joined lines") against statements that do not come from it, without a device: its
defaults are tests/mesh_ref.py; a convex solid hides none of its contour samples; the hidden samples of two occluded scenes
counted by a second statement of the rule, a loop over faces in Python floats; the outline of a finely tessellated sphere
comes back as one cycle of nearly its full length where the old definition keeps a fraction; every point a joined line skips
lies within the tolerance of it; polyhedra keep their lines; the limit of 256 segments; the start of a cycle; the refusals."""
import numpy as np
import pytest

import mesh_cases as MC
import mesh_join_cases as JC
import mesh_join_ref as JR
import mesh_ref as MR

_runs = {}


def runs_of(name, visibility):
    key = (name, visibility)
    if key not in _runs:
        v, f, views, scale = JC.case(name)
        mesh = MR.Mesh(v, f, MC.COS30)
        _runs[key] = [JR.view_runs(mesh, R, scale, MR.default_depth_tol(v), visibility) for R in views]
    return _runs[key]


_sphere = {}


def sphere_runs(subdivisions, scale, visibility):
    key = (subdivisions, scale, visibility)
    if key not in _sphere:
        v, f = MC.icosphere(subdivisions)
        _sphere[key] = JR.view_runs(MR.Mesh(v, f, MC.COS30), MC.GENERIC, np.float32(scale), MR.default_depth_tol(v), visibility)
    return _sphere[key]


def _total(lines):
    return float(np.hypot(lines[:, 2].astype(np.float64) - lines[:, 0], lines[:, 3].astype(np.float64) - lines[:, 1]).sum())


@pytest.mark.parametrize("name", ["cube-65", "l_prism", "occluded_cubes", "icosphere", "roof", "degenerate", "fence"])
def test_defaults_are_the_old_referee(name):
    v, f, views, scale = JC.case(name)
    mesh = MR.Mesh(v, f, MC.COS30)
    for min_length in (0.0, 2.0):
        want = MR.views_lines(mesh, views, scale, MR.default_depth_tol(v), min_length)
        got = JR.views_lines(mesh, views, scale, MR.default_depth_tol(v), min_length)
        assert got[1].tolist() == want[1].tolist() and got[0].tobytes() == want[0].tobytes()
        parts = [JR.lines_of_runs(r, min_length) for r in runs_of(name, "items")]
        assert np.concatenate(parts).tobytes() == want[0].tobytes()


@pytest.mark.parametrize("subdivisions,scale", [(2, 16.0), (3, 40.0), (4, 40.0)])
def test_a_sphere_hides_none_of_its_contour(subdivisions, scale):
    """Every sample of every candidate edge of a convex solid is visible; the item buffer's rule hides a third and more."""
    v, f = MC.icosphere(subdivisions)
    mesh = MR.Mesh(v, f, MC.COS30)
    X, Y, Z = MR.project(mesh.v, MC.GENERIC, np.float32(scale))
    box = MR.view_box(X, Y)
    D = MR.item_buffer(mesh, X, Y, Z, box)
    samples = visible = old = 0
    for e in np.nonzero(MR.candidates(mesh, X, Y))[0]:
        vis = JR.exact_visibility(mesh, X, Y, Z, e, MR.default_depth_tol(v))[0]
        samples += len(vis)
        visible += int(vis.sum())
        old += int(MR.edge_lines(mesh, X, Y, Z, box, D, e, MR.default_depth_tol(v), 0.0)[1].sum())
    assert samples > 100 and visible == samples
    assert old < 0.75 * samples


def _hidden_by_loop(mesh, R, scale, depth_tol):
    """(samples, hidden) of a view by the rule of the header stated a second time: a loop over samples and faces on Python floats
    made from the float32 projections and samples."""
    X, Y, Z = MR.project(mesh.v, R, scale)
    fx, fy, fz = ([float(t) for t in w] for w in (X, Y, Z))
    tris = mesh.f.tolist()

    def o(ax, ay, bx, by, cx, cy):
        return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    samples = hidden = 0
    for e in np.nonzero(MR.candidates(mesh, X, Y))[0]:
        A, B = (int(i) for i in mesh.everts[e])
        with np.errstate(all="ignore"):
            dx, dy, dz = X[B] - X[A], Y[B] - Y[A], Z[B] - Z[A]
            n = max(1, int(np.ceil(max(abs(dx), abs(dy)))))
            t = np.arange(n + 1).astype(np.float32) / np.float32(n)
            SX, SY, SZ = X[A] + t * dx, Y[A] + t * dy, Z[A] + t * dz
        own = set(int(q) for q in mesh.efaces[e])
        for k in range(n + 1):
            sx, sy, lim = float(SX[k]), float(SY[k]), float(SZ[k]) + float(depth_tol)
            samples += 1
            for f, (a, b, c) in enumerate(tris):
                if f in own or (k == 0 and A in (a, b, c)) or (k == n and B in (a, b, c)):
                    continue
                if not (min(fx[a], fx[b], fx[c]) <= sx <= max(fx[a], fx[b], fx[c]) and min(fy[a], fy[b], fy[c]) <= sy <= max(fy[a], fy[b], fy[c])):
                    continue
                area = o(fx[a], fy[a], fx[b], fy[b], fx[c], fy[c])
                if area == 0:
                    continue
                e0, e1, e2 = o(fx[b], fy[b], fx[c], fy[c], sx, sy), o(fx[c], fy[c], fx[a], fy[a], sx, sy), o(fx[a], fy[a], fx[b], fy[b], sx, sy)
                if not ((e0 >= 0 and e1 >= 0 and e2 >= 0) or (e0 <= 0 and e1 <= 0 and e2 <= 0)):
                    continue
                if (e0 * fz[a] + e1 * fz[b] + e2 * fz[c]) / area > lim:
                    hidden += 1
                    break
    return samples, hidden


@pytest.mark.parametrize("name", ["occluded_cubes", "fence"])
def test_hidden_counts_by_a_second_statement(name):
    v, f, views, scale = JC.case(name)
    mesh = MR.Mesh(v, f, MC.COS30)
    tol = MR.default_depth_tol(v)
    for R in views:
        X, Y, Z = MR.project(mesh.v, R, scale)
        samples = hidden = 0
        for e in np.nonzero(MR.candidates(mesh, X, Y))[0]:
            vis = JR.exact_visibility(mesh, X, Y, Z, e, tol)[0]
            samples += len(vis)
            hidden += int((~vis).sum())
        assert (samples, hidden) == _hidden_by_loop(mesh, R, scale, tol)
        assert 0 < hidden < samples
    if name == "fence":     # the sheet's long edges behind 40 slats, and nothing of a slat hidden
        assert samples == 4996 and samples - hidden == 3957


def test_the_outline_of_a_fine_sphere_comes_back():
    outline = 2 * np.pi * 40.0
    lines, info, pre = JR.lines_of_runs(sphere_runs(4, 40.0, "exact"), 2.0, 0.5, want_chains=True)
    assert len(info) == 1
    members, P, emitted = info[0]
    assert len(members) == len(pre) and P[0] == P[-1]       # one cycle through every run
    kept = _total(lines)
    assert 0.9 * outline <= kept <= outline
    assert len(lines) < len(pre) / 3
    old = JR.lines_of_runs(sphere_runs(4, 40.0, "items"), 2.0)
    assert _total(old) < 0.25 * kept
    # joining alone does not help: the old rule leaves the contour in pieces
    joined_old, info_old, _ = JR.lines_of_runs(sphere_runs(4, 40.0, "items"), 2.0, 0.5, want_chains=True)
    assert len(info_old) > 10 and _total(joined_old) < 0.5 * kept


def _check_within(info, tol):
    """Every chain point a line skips projects inside the line and lies within tol of it, up to float32 rounding of the
    products (relative 2^-23 of lengths up to the line's own and the coordinates' size)."""
    checked = 0
    for members, P, emitted in info:
        pts = np.array(P, dtype=np.float64)
        at = 0
        spans = JR.simplify_spans(P, tol)
        assert len(spans) == len(emitted)
        for (a, j), ln in zip(spans, emitted):
            assert a == at and j > a and ln == (P[a][0], P[a][1], P[j][0], P[j][1])
            d = pts[j] - pts[a]
            L = np.hypot(*d)
            slack = 1e-6 * (L + np.abs(pts).max())
            assert j - a <= JR.MAX_SPAN_SEGMENTS
            for i in range(a + 1, j):
                w = pts[i] - pts[a]
                s, c = (d @ w) / L, (d[0] * w[1] - d[1] * w[0]) / L
                assert -slack <= s <= L + slack and abs(c) <= tol + slack, (a, i, j, s, c)
                checked += 1
            at = j
        assert at == len(pts) - 1
    return checked


@pytest.mark.parametrize("name", JC.NAMES)
def test_skipped_points_lie_within_the_tolerance(name):
    checked = 0
    for visibility in ("items", "exact"):
        for tol in (0.5, 0.0):
            for runs in runs_of(name, visibility):
                checked += _check_within(JR.lines_of_runs(runs, 0.0, tol, want_chains=True)[1], tol)
    assert checked > 0 or name in ("triangle-none", "triangle-one", "cube-centres", "cube-65", "cube-2000", "tetrahedron", "open_square",
                                   "triangle-257x3", "triangle-3x257", "l_prism", "occluded_cubes", "roof", "fence", "fence-turned")


@pytest.mark.parametrize("mesh_name", ["cube", "l_prism", "notched_prism"])
def test_polyhedra_keep_their_lines(mesh_name):
    v, f = {"cube": MC.cube, "l_prism": MC.l_prism, "notched_prism": MC.notched_prism}[mesh_name]()
    mesh = MR.Mesh(v, f, MC.COS30)
    runs = JR.view_runs(mesh, MC.GENERIC, np.float32(20.3), MR.default_depth_tol(v), "exact")
    plain, joined = JR.lines_of_runs(runs, 2.0), JR.lines_of_runs(runs, 2.0, 0.5)
    assert len(plain) == len(joined) >= 9
    if mesh_name == "cube":
        assert len(joined) == 9         # three faces towards the viewer: nine edges
    # the same segments, whichever way round, their ends at the projected vertices instead of the last samples
    both = np.concatenate([plain, plain[:, [2, 3, 0, 1]]]).astype(np.float64)
    for ln in joined.astype(np.float64):
        assert np.abs(both - ln).max(axis=1).min() <= 1e-3


def test_a_joined_line_replaces_at_most_256_segments():
    runs = runs_of("ribbon", "exact")[0]            # the identity view: borders of 300 collinear edges of 1.5 pixels
    assert len(runs) == 2 * JC.RIBBON_EDGES + 2
    for tol in (0.0, 0.5):
        lines, info, _ = JR.lines_of_runs(runs, 2.0, tol, want_chains=True)
        assert len(info) == 1 and info[0][1][0] == info[0][1][-1]      # the boundary is one cycle
        length = np.hypot(lines[:, 2] - lines[:, 0], lines[:, 3] - lines[:, 1])
        assert length.max() == JR.MAX_SPAN_SEGMENTS * JC.RIBBON_STEP
        assert int((length == JR.MAX_SPAN_SEGMENTS * JC.RIBBON_STEP).sum()) == 2
        assert abs(float(length.sum()) - (2 * JC.RIBBON_EDGES + 4) * JC.RIBBON_STEP) < 1e-3


@pytest.mark.parametrize("name", ["icosphere", "icosphere3_bumped", "ribbon", "cube-65"])
def test_a_cycle_starts_with_its_lowest_line_and_chains_are_in_order(name):
    cycles = 0
    for runs in runs_of(name, "exact"):
        info = JR.lines_of_runs(runs, 0.0, 0.5, want_chains=True)[1]
        firsts = [members[0][0] for members, _, _ in info]
        assert firsts == sorted(firsts)
        assert sorted(l for members, _, _ in info for l, _ in members) == list(range(len(runs)))
        for members, P, _ in info:
            if len(members) > 1 and P[0] == P[-1]:
                cycles += 1
                assert members[0] == (min(l for l, _ in members), 0)
            else:
                assert members[0][0] == min(members[0][0], members[-1][0])
    assert cycles > 0 or name in ("cube-65", "icosphere3_bumped")      # (the bumps hide parts of the outline: paths only)


def test_refusals():
    v, f = MC.cube()
    mesh = MR.Mesh(v, f, MC.COS30)
    with pytest.raises(ValueError):
        JR.view_lines(mesh, MC.IDENTITY, np.float32(10), 0.0, 2.0, "exact", float("nan"))
    with pytest.raises(ValueError):
        JR.view_lines(mesh, MC.IDENTITY, np.float32(10), 0.0, 2.0, "exact", float("inf"))
    with pytest.raises(ValueError):
        JR.view_lines(mesh, MC.IDENTITY, np.float32(10), 0.0, 2.0, "both")
