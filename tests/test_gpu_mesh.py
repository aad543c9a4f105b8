"""The mesh templates on the device (include/fdcm.h, "Templates from a mesh") against the referee (tests/mesh_ref.py), byte for
byte: every view's pixel box and item buffer, the offsets and lines of every case of tests/mesh_cases.py at both least
lengths, both depth tolerances and three crease angles; lists of views against the views one call each; repeated calls;
several parts and FDCM_POISON in fresh processes (tools/mesh_probe.py); no views; and the views the call refuses.  Past one block
per view and one pass per loop: more than 128 listed faces and more than 256 block sums in one part, a mesh of 3 vertex and 8
edge blocks in lists and in writing runs that start mid-part, 41 lines on one edge, and parts cut by the 512 MB limit
(tests/test_mesh_definition.py states on the referee alone that the shapes used here do reach those paths)."""
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


_views_ref = {}


def views_ref(mesh_name, n_views, scale, min_length):
    """MR.views_lines of view_rotations(n_views, hemisphere=False) at the default tolerance, computed once."""
    key = (mesh_name, n_views, scale, min_length)
    if key not in _views_ref:
        from openfdcm_amd.engine import view_rotations
        v, f = MC.MESHES[mesh_name]()
        _views_ref[key] = MR.views_lines(MR.Mesh(v, f, MC.COS30), view_rotations(n_views, hemisphere=False), np.float32(scale),
                                         MR.default_depth_tol(v), min_length)
    return _views_ref[key]


def _same(got, want):
    assert got[1].tolist() == want[1].tolist()
    assert got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes()


def test_more_listed_faces_than_one_pass_of_the_big_raster(engine):
    """432 listed (view, face) pairs in one part are 6912 units on k_mesh_raster_big's grid of 2048: workgroups make up to four
    passes (test_mesh_definition.test_forty_views_of_the_cubes_list_432_faces counts the pairs)."""
    v, f = MC.occluded_cubes()
    want = views_ref("occluded_cubes", 40, 40.0, 2.0)
    assert len(want[0]) == 688
    _same(engine.mesh_view_lines(engine.Mesh(v, f), engine.view_rotations(40, hemisphere=False), 40.0, None, 2.0), want)


def test_more_block_sums_than_one_pass_of_the_scan(engine):
    """300 (view, block) pairs: the second pass of k_mesh_scan adds a carry of 1321.  Then 40 views of 8 edge blocks: 320 pairs,
    and the copy of every view's first sum strides over 8."""
    v, f = MC.tetrahedron()
    want = views_ref("tetrahedron", 300, 9.3, 0.0)
    assert len(want[0]) == 1553 and want[1][256] == 1321
    _same(engine.mesh_view_lines(engine.Mesh(v, f), engine.view_rotations(300, hemisphere=False), 9.3, None, 0.0), want)
    v, f = MC.icosphere3_bumped()
    want = views_ref("icosphere3_bumped", 40, 33.7, 0.0)
    assert np.all(np.diff(want[1]) > 0)
    _same(engine.mesh_view_lines(engine.Mesh(v, f), engine.view_rotations(40, hemisphere=False), 33.7, None, 0.0), want)


def test_a_refused_view_late_in_a_long_list(engine):
    from openfdcm_amd import _capi
    v, f = MC.tetrahedron()
    mesh = engine.Mesh(v, f)
    views = engine.view_rotations(300, hemisphere=False)
    bad = views.copy()
    bad[299] = np.diag([5000.0, 1.0, 1.0])
    assert MR.view_box(*MR.project(v, bad[299], np.float32(9.3))[:2]) is None
    with pytest.raises(_capi.FdcmError, match="view 299 spans more than 4096"):
        engine.mesh_view_lines(mesh, bad, 9.3, None, 0.0)
    want = views_ref("tetrahedron", 300, 9.3, 0.0)
    got = engine.mesh_view_lines(mesh, views[:299], 9.3, None, 0.0)     # the refusal left nothing behind
    assert got[1].tolist() == want[1][:300].tolist() and got[0].tobytes() == want[0][:want[1][299]].tobytes()


def test_lists_of_views_of_a_mesh_of_several_blocks(engine):
    v, f = MC.icosphere3_bumped()
    mesh = engine.Mesh(v, f)
    views = engine.view_rotations(9, hemisphere=False)
    single = [engine.mesh_view_lines(mesh, R, 33.7, None, 0.0)[0] for R in views]
    assert all(len(s) > 0 for s in single)
    a = engine.mesh_view_lines(mesh, views, 33.7, None, 0.0)
    assert a[1].tolist() == np.concatenate([[0], np.cumsum([len(s) for s in single])]).tolist()
    assert a[0].tobytes() == np.concatenate(single).tobytes()
    for _ in range(2):
        b = engine.mesh_view_lines(mesh, views, 33.7, None, 0.0)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


SQUARE_4095 = [[-2047.5, -2047.5, 2047.5, -2047.5], [-2047.5, -2047.5, -2047.5, 2047.5], [2047.5, -2047.5, 2047.5, 2047.5],
               [-2047.5, 2047.5, 2047.5, 2047.5]]   # the referee's lines of the cube at 4095 (test_mesh_definition computes them)


def test_parts_cut_by_the_byte_limit(engine):
    """Five item buffers of 128 MB: parts of 3 and 2 views under the 512 MB the header states, with no switch set."""
    v, f = MC.cube()
    box = MR.view_box(*MR.project(v, MC.IDENTITY, np.float32(4095.0))[:2])
    one = (box[2] - box[0] + 1) * (box[3] - box[1] + 1) * 8
    assert 5 * one > 512 << 20 and 4 * one >= 512 << 20 > 3 * one + (1 << 20)    # (the megabyte: the list and the counts)
    assert "FDCM_MESH_PART" not in os.environ
    rec, off = engine.mesh_view_lines(engine.Mesh(v, f), np.stack([MC.IDENTITY] * 5), 4095.0)
    assert off.tolist() == [0, 4, 8, 12, 16, 20]
    assert rec.tobytes() == np.array(SQUARE_4095 * 5, dtype=np.float32).tobytes()


@pytest.mark.parametrize("name", ["fence", "fence-turned"])
def test_fence_edges_carry_41_lines_each(engine, name):
    v, f, views, scale = MC.case(name)
    ref = MR.Mesh(v, f, MC.COS30)
    got, off = engine.mesh_view_lines(engine.Mesh(v, f), views, scale, None, 0.0)
    assert off.tolist() == [0, 244]
    (X, Y, Z, box, D), = raster(name)
    at = 0
    long_edges = 0
    for e in np.nonzero(MR.candidates(ref, X, Y))[0]:
        lines = MR.edge_lines(ref, X, Y, Z, box, D, e, MR.default_depth_tol(v), 0.0)[0]
        if ref.everts[e].tolist() in ([0, 1], [2, 3]):
            assert len(lines) == 41
            assert got[at:at + 41].tobytes() == np.array(lines, dtype=np.float32).tobytes(), ref.everts[e]
            long_edges += 1
        at += len(lines)
    assert long_edges == 2 and at == 244


def _probe(env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}
    out = subprocess.run([sys.executable, PROBE], capture_output=True, text=True, timeout=120, env={**clean, **env})
    assert out.returncode == 0, out.stdout + out.stderr
    return [l for l in out.stdout.splitlines() if l.startswith("mesh_probe ")][-1].split()


def test_parts_and_poison_in_fresh_processes(engine):
    """tools/mesh_probe.py in fresh processes, one after another, each under its own time limit; nothing is started after a
    failure (an assertion ends the test).  65 views in parts of 7 (FDCM_MESH_PART, read once per process) are ten parts; in
    parts of 2 the room of a writing run is 32 lines, so every view of the bumped icosphere (8 edge blocks) is a writing run of
    its own, the second of a part starting at block 8.  The digests equal this process's own, whose lines of that mesh are the
    referee's."""
    spec = __import__("importlib.util").util.spec_from_file_location("mesh_probe", PROBE)
    probe = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    results = probe.results()
    digest, n_lines = probe.digest(results)
    assert n_lines > 500
    name, n, scale, min_length = probe.CALLS[2]
    want = views_ref(name, n, scale, min_length)
    assert name == "icosphere3_bumped" and np.all(np.diff(want[1]) > 32)
    _same(results[2], want)
    for env in ({"FDCM_MESH_PART": "7"}, {"FDCM_MESH_PART": "2"}, {"FDCM_POISON": "0"}, {"FDCM_POISON": "1"}, {"FDCM_POISON": "1", "FDCM_MESH_PART": "1"}):
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
