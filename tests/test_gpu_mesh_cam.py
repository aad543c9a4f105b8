"""The pinhole views of the mesh templates on the device (include/fdcm.h, "Templates from a mesh: pinhole views") against the
referee (tests/mesh_cam_ref.py): the pixel box and the item buffer key for key, offsets and lines byte for byte in the modes
{items, exact} x {no joining, 0.5} on every case of tests/mesh_cam_cases.py; a list of views with mixed positions against the
views one call each; repeated calls; several parts and FDCM_POISON in fresh processes (tools/mesh_cam_probe.py); the scale
identity, which needs no referee; the refusal of a view with a vertex inside `near`; and the default call, which keeps its
bytes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_cam_cases as CC
import mesh_cam_ref as CR
import mesh_cases as MC
import mesh_ref as MR
from helpers import ROOT

pytestmark = pytest.mark.gpu
PROBE = os.path.join(ROOT, "tools", "mesh_cam_probe.py")
MODES = [("items", None), ("items", 0.5), ("exact", None), ("exact", 0.5)]


@pytest.fixture(scope="module")
def engine():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    from openfdcm_amd import engine
    return engine


@pytest.mark.parametrize("name", CC.NAMES)
def test_item_buffer_is_the_referees(engine, name):
    v, f, views, pos, focal = CC.case(name)
    mesh = engine.Mesh(v, f)
    seen = 0
    for R, t, (box, D) in zip(views, pos, CC.ref_raster(name)):
        got_box, keys = engine.mesh_view_items(mesh, R, focal=focal, positions=t)
        assert got_box == box
        assert keys.shape == D.shape and np.array_equal(keys, D), (name, int((keys != D).sum()))
        seen += int((D != 0).sum())
    assert seen > 0


@pytest.mark.parametrize("name", CC.NAMES)
def test_lines_are_the_referees(engine, name):
    v, f, views, pos, focal = CC.case(name)
    mesh = engine.Mesh(v, f)
    for visibility, tol in MODES:
        for min_length in (2.0, 0.0):
            want, want_off = CC.ref_lines(name, visibility, tol, min_length)
            got, off = engine.mesh_view_lines(mesh, views, None, None, min_length, visibility, tol, focal=focal, positions=pos)
            assert off.tolist() == want_off.tolist(), (name, visibility, tol, min_length)
            assert got.tobytes() == want.tobytes(), (name, visibility, tol, min_length)
            assert len(want) >= len(views)
    tm = engine.templates_from_mesh(mesh, views, focal=focal, positions=pos, visibility="exact", join_tolerance=0.5)
    want, want_off = CC.ref_lines(name, "exact", 0.5, 2.0)
    assert [t.shape for t in tm] == [(4, want_off[i + 1] - want_off[i]) for i in range(len(views))]
    assert np.concatenate(tm, axis=1).T.tobytes() == want.tobytes()


def test_lists_of_views_are_the_views_one_call_each_and_calls_repeat(engine):
    """7 views of the bumped icosphere (8 edge blocks a view) at positions that differ from view to view: a view takes its own
    position wherever it stands in the list, in a part or a run."""
    v, f = MC.icosphere3_bumped()
    mesh = engine.Mesh(v, f)
    views = engine.view_rotations(7, hemisphere=False)
    g = CC.diagonal(v)
    k = np.arange(7)
    pos = (np.stack([0.3 * np.cos(2.0 * k) * (k % 2), 0.25 * np.sin(k), -(3.0 + 0.5 * k)], axis=1) * g).astype(np.float32)
    for visibility, tol in MODES:
        single = [engine.mesh_view_lines(mesh, R, None, None, 2.0, visibility, tol, focal=1000.0, positions=t)[0] for R, t in zip(views, pos)]
        assert all(len(s) > 0 for s in single)
        a = engine.mesh_view_lines(mesh, views, None, None, 2.0, visibility, tol, focal=1000.0, positions=pos)
        assert a[1].tolist() == np.concatenate([[0], np.cumsum([len(s) for s in single])]).tolist()
        assert a[0].tobytes() == np.concatenate(single).tobytes()
        b = engine.mesh_view_lines(mesh, views, None, None, 2.0, visibility, tol, focal=1000.0, positions=pos)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # one position for all views is that position per view
    one = engine.mesh_view_lines(mesh, views[:3], focal=1000.0, positions=pos[2])
    rows = engine.mesh_view_lines(mesh, views[:3], focal=1000.0, positions=np.tile(pos[2], (3, 1)))
    assert len(one[0]) > 0 and one[0].tobytes() == rows[0].tobytes() and one[1].tolist() == rows[1].tolist()


def _probe(env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}
    out = subprocess.run([sys.executable, PROBE], capture_output=True, text=True, timeout=120, env={**clean, **env})
    assert out.returncode == 0, out.stdout + out.stderr
    return [l for l in out.stdout.splitlines() if l.startswith("mesh_cam_probe ")][-1].split()


def test_parts_and_poison_in_fresh_processes(engine):
    """tools/mesh_cam_probe.py in fresh processes, one after another, each under its own time limit; nothing is started after a
    failure (an assertion ends the test).  In parts of 2 views the positions of a part begin at its first view, and a writing
    run holds 32 lines, so every view of the bumped icosphere is a run of its own with its own position.  The digests equal
    this process's own."""
    spec = __import__("importlib.util").util.spec_from_file_location("mesh_cam_probe", PROBE)
    probe = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    digest, n_lines = probe.digest(probe.results())
    assert n_lines > 500
    for env in ({"FDCM_MESH_PART": "2"}, {"FDCM_POISON": "1"}):
        line = _probe(env)
        assert line[1] == digest and int(line[3]) == n_lines, (env, line)


@pytest.mark.parametrize("name", ["occluded_cubes", "notched_prism", "icosphere"])
def test_scale_identity(engine, name):
    """Vertices, positions, near and the depth tolerance all times 2: every projected X and Y is the same float (a power of two
    scales P and d exactly, Z = 1 / d halves exactly, and both sides of either tolerance compare halve), so the lines are the
    same bytes.  No referee is needed."""
    v, f, views, pos, focal = CC.case(name)
    a, b = engine.Mesh(v, f), engine.Mesh(v * np.float32(2.0), f)
    tol, near = MR.default_depth_tol(v), CR.default_near(v)
    for visibility, join in MODES:
        one = engine.mesh_view_lines(a, views, None, tol, 2.0, visibility, join, focal=focal, positions=pos, near=near)
        two = engine.mesh_view_lines(b, views, None, tol * np.float32(2.0), 2.0, visibility, join, focal=focal,
                                     positions=pos * np.float32(2.0), near=near * np.float32(2.0))
        assert len(one[0]) > 0 and one[1].tolist() == two[1].tolist() and one[0].tobytes() == two[0].tobytes()


def test_refusals(engine):
    from openfdcm_amd import _capi
    v, f = MC.cube()
    mesh = engine.Mesh(v, f)
    views = np.stack([MC.IDENTITY, MC.GENERIC, MC.GENERIC2])
    far = np.float32([0, 0, -6.0])
    # view 1 of 3 has its nearest vertex at 0.2 (GENERIC turns a corner of the cube towards the camera), inside near = 0.25
    X, Y, Z, d = CR.project(v, MC.GENERIC, (0.0, 0.0, -1.0), 100.0)
    close = np.float32([0, 0, -(1.0 - float(d.min()) + 0.2)])
    pos = np.stack([far, close, far])
    for visibility, tol in MODES[::3]:
        with pytest.raises(_capi.FdcmError, match="view 1 .*nearer than"):
            engine.mesh_view_lines(mesh, views, None, None, 2.0, visibility, tol, focal=100.0, positions=pos, near=0.25)
    with pytest.raises(_capi.FdcmError, match="view 0 .*nearer than"):
        engine.mesh_view_items(mesh, MC.GENERIC, focal=100.0, positions=close, near=0.25)
    ok = engine.mesh_view_lines(mesh, views, focal=100.0, positions=pos, near=0.15)     # the same views a little further from near
    assert np.all(np.diff(ok[1]) > 0)
    # a vertex behind the camera (d < 0) and one in its plane (d = 0, Z infinite) are inside any near
    for z in (-0.3, -0.5):
        with pytest.raises(_capi.FdcmError, match="view 0 "):
            engine.mesh_view_lines(mesh, MC.IDENTITY, focal=100.0, positions=(0, 0, z), near=1e-6)
    # an oversized box is still refused with its index
    with pytest.raises(_capi.FdcmError, match="view 2 spans more than 4096"):
        engine.mesh_view_lines(mesh, views, focal=30000.0, positions=np.stack([far * 10, far * 10, far]))
    # before any GPU work
    for kw, what in ((dict(focal=0.0), "focal"), (dict(focal=float("inf")), "focal"), (dict(near=0.0), "near"),
                     (dict(near=float("nan")), "near"), (dict(positions=(0, 0, 1.0)), "position 0"), (dict(positions=(0, 0, 0.0)), "position 0"),
                     (dict(positions=(float("nan"), 0, -5.0)), "position 0"), (dict(join_tolerance=float("nan")), "join_tolerance"),
                     (dict(visibility=2), "visibility"), (dict(depth_tolerance=-1.0), "depth_tol")):
        args = dict(dict(focal=100.0, positions=far, near=0.1), **kw)
        with pytest.raises(_capi.FdcmError, match=what):
            engine.mesh_view_lines(mesh, MC.IDENTITY, **args)
    rec, off = engine.mesh_view_lines(mesh, np.zeros((0, 3, 3), dtype=np.float32), focal=100.0, positions=np.zeros((0, 3), dtype=np.float32))
    assert rec.shape == (0, 4) and off.tolist() == [0]


@pytest.mark.parametrize("name", ["l_prism", "icosphere", "fence"])
def test_default_call_keeps_its_bytes(engine, name):
    """templates_from_mesh(mesh, views, scale) is fdcm_mesh_view_lines, and the orthographic referee's lines."""
    from openfdcm_amd import _capi
    v, f, views, scale = MC.case(name)
    mesh = engine.Mesh(v, f)
    r = np.ascontiguousarray(views, dtype=np.float32)
    offsets = np.zeros(len(r) + 1, dtype=np.int64)
    out = C.POINTER(C.c_float)()
    _capi.check(_capi.lib().fdcm_mesh_view_lines(mesh._h, _capi.fptr(r), len(r), float(scale), float(mesh.default_depth_tolerance()), 2.0,
                                                 C.byref(out), offsets.ctypes.data_as(C.POINTER(C.c_int64))))
    n = int(offsets[-1])
    old = np.ctypeslib.as_array(out, shape=(n, 4)).copy()
    _capi.lib().fdcm_lines_free(out)
    tm = engine.templates_from_mesh(mesh, views, scale)
    assert n > 0 and [t.shape[1] for t in tm] == np.diff(offsets).tolist()
    assert np.concatenate(tm, axis=1).T.tobytes() == old.tobytes()
    want, want_off = MR.views_lines(MR.Mesh(v, f, MC.COS30), views, scale, MR.default_depth_tol(v), 2.0)
    assert offsets.tolist() == want_off.tolist() and old.tobytes() == want.tobytes()
    tm2 = engine.templates_from_mesh(mesh, views, scale=scale)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(tm, tm2))
