"""Exact visibility and joined lines of the mesh templates on the device (include/fdcm.h, "Templates from a mesh: exact visibility
and joined lines") against the referee (tests/mesh_join_ref.py), byte for byte in offsets and lines: every case of
tests/mesh_cases.py and the ribbon of tests/mesh_join_cases.py in the modes {items, exact} x {no joining, 0.5}, and exact with
tolerance 0; the default call through the _ex entry against fdcm_mesh_view_lines; lists of views against the views one call
each; repeated calls; several parts and FDCM_POISON in fresh processes (tools/mesh_join_probe.py); the refusals.  The cases
reach: all 320 faces in one tile (icosphere-small), faces over tens of thousands of tiles (cube-2000), chains across 8 edge
blocks and 3 vertex blocks (icosphere3_bumped), 41 runs per edge with free ends inside the edge (fence), and joined lines cut at
256 segments (ribbon)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_cases as MC
import mesh_join_cases as JC
import mesh_join_ref as JR
import mesh_ref as MR
from helpers import ROOT

pytestmark = pytest.mark.gpu
PROBE = os.path.join(ROOT, "tools", "mesh_join_probe.py")
MODES = [("items", None), ("items", 0.5), ("exact", None), ("exact", 0.5), ("exact", 0.0)]


@pytest.fixture(scope="module")
def engine():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    from openfdcm_amd import engine
    return engine


_runs = {}


def ref_runs(name, visibility):
    """Per view of the case the referee's runs at the default tolerance: they depend on neither min_length nor the joining, so
    every mode of a case shares them."""
    key = (name, visibility)
    if key not in _runs:
        v, f, views, scale = JC.case(name)
        mesh = MR.Mesh(v, f, MC.COS30)
        _runs[key] = [JR.view_runs(mesh, R, scale, MR.default_depth_tol(v), visibility) for R in views]
    return _runs[key]


def ref_lines(name, visibility, tol, min_length):
    parts = [JR.lines_of_runs(r, min_length, tol) for r in ref_runs(name, visibility)]
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in parts], out=offsets[1:])
    return np.concatenate(parts).reshape(-1, 4), offsets


@pytest.mark.parametrize("name", JC.NAMES)
def test_lines_are_the_referees(engine, name):
    v, f, views, scale = JC.case(name)
    mesh = engine.Mesh(v, f)
    seen = 0
    for visibility, tol in MODES:
        for min_length in (2.0, 0.0):
            want, want_off = ref_lines(name, visibility, tol, min_length)
            got, off = engine.mesh_view_lines(mesh, views, scale, None, min_length, visibility, tol)
            assert off.tolist() == want_off.tolist(), (name, visibility, tol, min_length)
            assert got.tobytes() == want.tobytes(), (name, visibility, tol, min_length)
            seen += len(want)
    assert seen > 0 or name == "triangle-none"
    tm = engine.templates_from_mesh(mesh, views, scale, visibility="exact", join_tolerance=0.5)
    want, want_off = ref_lines(name, "exact", 0.5, 2.0)
    assert [t.shape for t in tm] == [(4, want_off[i + 1] - want_off[i]) for i in range(len(views))]
    assert np.concatenate(tm, axis=1).T.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", ["l_prism", "icosphere", "fence", "ribbon"])
def test_default_call_through_ex_is_the_old_entry(engine, name):
    from openfdcm_amd import _capi
    v, f, views, scale = JC.case(name)
    mesh = engine.Mesh(v, f)
    tol = float(mesh.default_depth_tolerance())
    r = np.ascontiguousarray(views, dtype=np.float32)
    offsets = np.zeros(len(r) + 1, dtype=np.int64)
    out = C.POINTER(C.c_float)()
    _capi.check(_capi.lib().fdcm_mesh_view_lines(mesh._h, _capi.fptr(r), len(r), float(scale), tol, 2.0, C.byref(out),
                                                 offsets.ctypes.data_as(C.POINTER(C.c_int64))))
    n = int(offsets[-1])
    old = np.ctypeslib.as_array(out, shape=(n, 4)).copy()
    _capi.lib().fdcm_lines_free(out)
    got, off = engine.mesh_view_lines(mesh, views, scale, None, 2.0, "items", None)
    assert n > 0 and off.tolist() == offsets.tolist() and got.tobytes() == old.tobytes()
    want, want_off = MR.views_lines(MR.Mesh(v, f, MC.COS30), views, scale, MR.default_depth_tol(v), 2.0)
    assert off.tolist() == want_off.tolist() and got.tobytes() == want.tobytes()


def test_lists_of_views_are_the_views_one_call_each_and_calls_repeat(engine):
    v, f = MC.icosphere3_bumped()
    mesh = engine.Mesh(v, f)
    views = engine.view_rotations(7, hemisphere=False)
    for visibility, tol in MODES[1:4]:
        single = [engine.mesh_view_lines(mesh, R, 33.7, None, 2.0, visibility, tol)[0] for R in views]
        assert all(len(s) > 0 for s in single)
        a = engine.mesh_view_lines(mesh, views, 33.7, None, 2.0, visibility, tol)
        assert a[1].tolist() == np.concatenate([[0], np.cumsum([len(s) for s in single])]).tolist()
        assert a[0].tobytes() == np.concatenate(single).tobytes()
        b = engine.mesh_view_lines(mesh, views, 33.7, None, 2.0, visibility, tol)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _probe(env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}
    out = subprocess.run([sys.executable, PROBE], capture_output=True, text=True, timeout=120, env={**clean, **env})
    assert out.returncode == 0, out.stdout + out.stderr
    return [l for l in out.stdout.splitlines() if l.startswith("mesh_join_probe ")][-1].split()


def test_parts_and_poison_in_fresh_processes(engine):
    """tools/mesh_join_probe.py in fresh processes, one after another, each under its own time limit; nothing is started after
    a failure (an assertion ends the test).  In parts of 2 views the room of a writing run is 32 lines, so every view of the
    bumped icosphere is a writing run of its own, with its own link table and chain pass.  The digests equal this process's
    own."""
    spec = __import__("importlib.util").util.spec_from_file_location("mesh_join_probe", PROBE)
    probe = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    digest, n_lines = probe.digest(probe.results())
    assert n_lines > 500
    for env in ({}, {"FDCM_MESH_PART": "2"}, {"FDCM_POISON": "1"}):
        line = _probe(env)
        assert line[1] == digest and int(line[3]) == n_lines, (env, line)


def test_refusals(engine):
    from openfdcm_amd import _capi
    v, f = MC.cube()
    mesh = engine.Mesh(v, f)
    with pytest.raises(_capi.FdcmError, match="join_tolerance"):
        engine.mesh_view_lines(mesh, MC.IDENTITY, 10.0, join_tolerance=float("nan"))
    with pytest.raises(_capi.FdcmError, match="join_tolerance"):
        engine.templates_from_mesh(mesh, MC.IDENTITY, 10.0, join_tolerance=float("inf"))
    with pytest.raises(_capi.FdcmError, match="visibility"):
        engine.mesh_view_lines(mesh, MC.IDENTITY, 10.0, visibility=2)
    with pytest.raises(_capi.FdcmError, match="view 0 spans more than 4096"):
        engine.mesh_view_lines(mesh, MC.IDENTITY, 5000.0, visibility="exact", join_tolerance=0.5)
    rec, off = engine.mesh_view_lines(mesh, np.zeros((0, 3, 3), dtype=np.float32), 10.0, visibility="exact", join_tolerance=0.5)
    assert rec.shape == (0, 4) and off.tolist() == [0]
