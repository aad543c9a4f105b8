"""The mesh templates on the device (include/fdcm.h, "Templates from a mesh") against the referee (tests/mesh_ref.py), byte for
byte: every view's pixel box and item buffer, the offsets and lines of every case of tests/mesh_cases.py at both least
lengths, both depth tolerances and three crease angles; lists of views against the views one call each; repeated calls;
several parts and FDCM_POISON in fresh processes (tools/mesh_probe.py); no views; and the views the call refuses."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_cases as MC
import mesh_ref as MR
from helpers import ROOT

pytestmark = pytest.mark.gpu
PROBE = os.path.join(ROOT, "tools", "mesh_probe.py")
NAMES = [c[0] for c in MC.CASES]


@pytest.fixture(scope="module")
def engine():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    from openfdcm_amd import engine
    return engine


_raster = {}


def raster(name):
    """Per view of the case: the projection, the box and the referee's item buffer (they depend on no parameter)."""
    if name not in _raster:
        v, f, views, scale = MC.case(name)
        mesh = MR.Mesh(v, f, MC.COS30)
        out = []
        for R in views:
            X, Y, Z = MR.project(mesh.v, R, scale)
            box = MR.view_box(X, Y)
            out.append((X, Y, Z, box, MR.item_buffer(mesh, X, Y, Z, box)))
        _raster[name] = out
    return _raster[name]


def ref_lines(name, crease_cos, depth_tol, min_length):
    v, f, views, scale = MC.case(name)
    mesh = MR.Mesh(v, f, crease_cos)
    parts = []
    for X, Y, Z, box, D in raster(name):
        lines = []
        for e in np.nonzero(MR.candidates(mesh, X, Y))[0]:
            lines += MR.edge_lines(mesh, X, Y, Z, box, D, e, depth_tol, min_length)[0]
        parts.append(np.array(lines, dtype=np.float32).reshape(-1, 4))
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in parts], out=offsets[1:])
    return np.concatenate(parts).reshape(-1, 4), offsets


@pytest.mark.parametrize("name", NAMES)
def test_item_buffer_is_the_referees(engine, name):
    v, f, views, scale = MC.case(name)
    mesh = engine.Mesh(v, f)
    seen = 0
    for R, (_, _, _, box, D) in zip(views, raster(name)):
        got_box, keys = engine.mesh_view_items(mesh, R, scale)
        assert got_box == box
        assert keys.shape == D.shape and np.array_equal(keys, D), (name, int((keys != D).sum()))
        seen += int((D != 0).sum())
    assert seen > 0 or name == "triangle-none"
    if name == "triangle-one":
        assert seen == 1


@pytest.mark.parametrize("name", NAMES)
def test_lines_are_the_referees(engine, name):
    v, f, views, scale = MC.case(name)
    total = 0
    for crease_cos, angle in ((-1.0, np.pi), (MC.COS30, np.deg2rad(30.0)), (1.0, 0.0)):
        mesh = engine.Mesh(v, f, crease_angle=angle)
        assert np.array_equal(mesh.edges()[2], MR.Mesh(v, f, crease_cos).sharp)    # (cos(angle) is the referee's cosine)
        for depth_tol in (np.float32(0.0), MR.default_depth_tol(v)):
            for min_length in (0.0, 2.0):
                want, want_off = ref_lines(name, crease_cos, depth_tol, min_length)
                got, off = engine.mesh_view_lines(mesh, views, scale, depth_tol, min_length)
                assert off.tolist() == want_off.tolist(), (name, crease_cos, depth_tol, min_length)
                assert got.tobytes() == want.tobytes(), (name, crease_cos, depth_tol, min_length)
                total += len(want)
    assert total > 0
    tm = engine.templates_from_mesh(engine.Mesh(v, f), views, scale)
    want, want_off = ref_lines(name, MC.COS30, MR.default_depth_tol(v), 2.0)
    assert len(tm) == len(views) and all(t.shape == (4, want_off[i + 1] - want_off[i]) and t.dtype == np.float32 for i, t in enumerate(tm))
    assert np.concatenate(tm, axis=1).T.tobytes() == want.tobytes()


def test_lists_of_views_are_the_views_one_call_each(engine):
    v, f = MC.l_prism()
    mesh = engine.Mesh(v, f)
    views = engine.view_rotations(65, hemisphere=False)
    single = [engine.mesh_view_lines(mesh, R, 20.3, None, 0.0)[0] for R in views]
    ref = MR.Mesh(v, f, MC.COS30)
    for i in (0, 7, 64):
        assert single[i].tobytes() == MR.view_lines(ref, views[i], np.float32(20.3), MR.default_depth_tol(v), 0.0).tobytes()
    for n in (1, 2, 65):
        got, off = engine.mesh_view_lines(mesh, views[:n], 20.3, None, 0.0)
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(s) for s in single[:n]])]).tolist()
        assert got.tobytes() == np.concatenate(single[:n]).tobytes()
    a = engine.mesh_view_lines(mesh, views, 20.3, None, 0.0)
    for _ in range(2):      # the same call: the same bytes
        b = engine.mesh_view_lines(mesh, views, 20.3, None, 0.0)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _probe(env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}
    out = subprocess.run([sys.executable, PROBE], capture_output=True, text=True, timeout=120, env={**clean, **env})
    assert out.returncode == 0, out.stdout + out.stderr
    return [l for l in out.stdout.splitlines() if l.startswith("mesh_probe ")][-1].split()


def test_parts_and_poison_in_fresh_processes(engine):
    """tools/mesh_probe.py in fresh processes, one after another, each under its own time limit; nothing is started after a
    failure (an assertion ends the test).  65 views in parts of 7 (FDCM_MESH_PART, read once per process) are ten parts; the
    digests equal this process's own."""
    spec = __import__("importlib.util").util.spec_from_file_location("mesh_probe", PROBE)
    probe = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    digest, n_lines = probe.run()
    assert n_lines > 500
    for env in ({"FDCM_MESH_PART": "7"}, {"FDCM_POISON": "0"}, {"FDCM_POISON": "1"}, {"FDCM_POISON": "1", "FDCM_MESH_PART": "1"}):
        line = _probe(env)
        assert line[1] == digest and int(line[3]) == n_lines, (env, line)


def test_no_views_and_refused_views(engine):
    from openfdcm_amd import _capi
    v, f = MC.cube()
    mesh = engine.Mesh(v, f)
    rec, off = engine.mesh_view_lines(mesh, np.zeros((0, 3, 3), dtype=np.float32), 10.0)
    assert rec.shape == (0, 4) and off.tolist() == [0] and engine.templates_from_mesh(mesh, np.zeros((0, 3, 3)), 10.0) == []
    views = np.stack([MC.IDENTITY, MC.GENERIC, MC.IDENTITY])
    assert MR.view_box(*MR.project(v, MC.IDENTITY, np.float32(4095.0))[:2]) is not None
    rec, off = engine.mesh_view_lines(mesh, MC.IDENTITY, 4095.0)                       # 4096 pixels on a side: the limit
    assert off[0] == 0 and off[1] == len(rec) >= 4
    assert MR.view_box(*MR.project(v, MC.GENERIC, np.float32(4095.0))[:2]) is None
    with pytest.raises(_capi.FdcmError, match="view 1 spans more than 4096"):
        engine.mesh_view_lines(mesh, views, 4095.0)
    with pytest.raises(_capi.FdcmError, match="view 0 spans more than 4096"):
        engine.mesh_view_lines(mesh, views, 3e37)       # coordinates beyond 2^30, and infinities behind them
    with pytest.raises(_capi.FdcmError, match="view 0 spans more than 4096"):
        engine.mesh_view_items(mesh, MC.IDENTITY, 5000.0)
    # a view that squeezes the mesh into one point is fine: one pixel, no line longer than 0
    rec, off = engine.mesh_view_lines(mesh, np.zeros((1, 3, 3), dtype=np.float32), 10.0, None, 0.0)
    assert off.tolist() == [0, 0]
