"""CPU-only checks of the mesh entry points of the C ABI (include/fdcm.h, "Templates from a mesh"): every argument error is
FDCM_EINVAL with a message before any device work, the edge table and the sharp flags are the referee's (tests/mesh_ref.py),
and the two pure-numpy helpers of the Python layer do what their documentation says.  No call here reaches a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_cases as MC
import mesh_ref as MR

EINVAL = -1
I32P, U8P, U64P, I64P = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def _create(capi, v, f, crease_cos=MC.COS30, n_vertices=None, n_faces=None, out=True):
    h = C.c_void_p()
    rc = capi.lib().fdcm_mesh_create(None if v is None else capi.fptr(v), len(v) if n_vertices is None else n_vertices,
                                     None if f is None else f.ctypes.data_as(I32P), len(f) if n_faces is None else n_faces,
                                     crease_cos, C.byref(h) if out else None)
    return rc, h


V, F = MC.cube()
CREATE_ERRORS = [
    (dict(v=None, n_vertices=8), "vertices is null"), (dict(f=None, n_faces=12), "faces is null"), (dict(out=False), "out is null"),
    (dict(n_vertices=0), "n_vertices"), (dict(n_vertices=-3), "n_vertices"), (dict(n_vertices=(1 << 22) + 1), "n_vertices"),
    (dict(n_faces=0), "n_faces"), (dict(n_faces=(1 << 22) + 1), "n_faces"),
    (dict(crease_cos=1.5), "crease_cos"), (dict(crease_cos=-1.01), "crease_cos"), (dict(crease_cos=float("nan")), "crease_cos"),
    (dict(n_vertices=7), "index outside"),
    (dict(f=np.array([[0, 1, -1]], dtype=np.int32)), "index outside"),
    (dict(v=np.where(np.arange(24).reshape(8, 3) == 13, np.float32("nan"), V).astype(np.float32)), "vertex 4 is not finite"),
    (dict(v=np.where(np.arange(24).reshape(8, 3) == 2, np.float32("inf"), V).astype(np.float32)), "vertex 0 is not finite"),
]


@pytest.mark.parametrize("kw,what", CREATE_ERRORS, ids=lambda v: str(v)[:60])
def test_create_argument_errors(capi, kw, what):
    rc, h = _create(capi, **dict(dict(v=V, f=F), **kw))
    assert rc == EINVAL and not h and what in _err(capi), _err(capi)


def test_non_manifold_mesh_is_refused(capi):
    rc, h = _create(capi, *MC.non_manifold())
    assert rc == EINVAL and not h and "non-manifold edge (0, 1)" in _err(capi)


@pytest.fixture(scope="module")
def cube(capi):
    rc, h = _create(capi, V, F)
    assert rc == 0 and h
    yield h
    assert capi.lib().fdcm_mesh_free(h) == 0


def _view_lines(capi, mesh, views=MC.IDENTITY, n_views=1, scale=10.0, depth_tol=0.0, min_length=2.0, lines=True, offsets=True):
    out, off = C.POINTER(C.c_float)(), np.full(max(n_views, 0) + 1, -7, dtype=np.int64)
    rc = capi.lib().fdcm_mesh_view_lines(mesh, None if views is None else capi.fptr(views), n_views, scale, depth_tol, min_length,
                                         C.byref(out) if lines else None, off.ctypes.data_as(I64P) if offsets else None)
    assert not out
    return rc, off


VIEW_ERRORS = [
    (dict(mesh=None), "mesh is null"), (dict(views=None), "views is null"), (dict(lines=False), "lines_out is null"),
    (dict(offsets=False), "offsets_out is null"), (dict(n_views=-1), "n_views"), (dict(n_views=65537), "n_views"),
    (dict(scale=0.0), "scale"), (dict(scale=-2.0), "scale"), (dict(scale=float("inf")), "scale"), (dict(scale=float("nan")), "scale"),
    (dict(depth_tol=-1e-6), "depth_tol"), (dict(depth_tol=float("nan")), "depth_tol"), (dict(depth_tol=float("inf")), "depth_tol"),
    (dict(min_length=-1.0), "min_length"), (dict(min_length=float("inf")), "min_length"), (dict(min_length=float("nan")), "min_length"),
    (dict(views=np.stack([MC.IDENTITY, np.where(np.eye(3) == 1, np.float32("nan"), MC.GENERIC)]).astype(np.float32), n_views=2),
     "view 1 has an entry that is not finite"),
]


@pytest.mark.parametrize("kw,what", VIEW_ERRORS, ids=lambda v: str(v)[:60])
def test_view_lines_argument_errors(capi, cube, kw, what):
    kw = dict(kw)
    rc, off = _view_lines(capi, kw.pop("mesh", cube), **kw)
    assert rc == EINVAL and what in _err(capi), _err(capi)
    assert np.all(off == -7)      # a refused call writes nothing


def test_zero_views_are_no_lines_and_no_device(capi, cube):
    rc, off = _view_lines(capi, cube, n_views=0)
    assert rc == 0 and off.tolist() == [0]
    rc, off = _view_lines(capi, cube, views=None, n_views=0)
    assert rc == 0 and off.tolist() == [0]


def test_view_items_argument_errors(capi, cube):
    lib = capi.lib()
    box = np.zeros(4, dtype=np.int32)
    keys = np.zeros(4, dtype=np.uint64)
    view = capi.fptr(MC.IDENTITY)
    for args, what in (((None, view, 1.0, box.ctypes.data_as(I32P), keys.ctypes.data_as(U64P), 4), "mesh is null"),
                       ((cube, None, 1.0, box.ctypes.data_as(I32P), keys.ctypes.data_as(U64P), 4), "view is null"),
                       ((cube, view, 1.0, None, keys.ctypes.data_as(U64P), 4), "box_out is null"),
                       ((cube, view, 0.0, box.ctypes.data_as(I32P), keys.ctypes.data_as(U64P), 4), "scale"),
                       ((cube, view, 1.0, box.ctypes.data_as(I32P), keys.ctypes.data_as(U64P), -1), "capacity")):
        assert lib.fdcm_mesh_view_items(*args) == EINVAL and what in _err(capi), (what, _err(capi))
    assert lib.fdcm_mesh_info(None, None, None, None) == EINVAL and lib.fdcm_mesh_edges(None, None, None, None) == EINVAL
    assert lib.fdcm_mesh_free(None) == 0


@pytest.mark.parametrize("name", sorted(MC.MESHES))
@pytest.mark.parametrize("crease_cos", [-1.0, MC.COS30, 1.0])
def test_edge_table_is_the_referees(capi, name, crease_cos):
    v, f = MC.MESHES[name]()
    ref = MR.Mesh(v, f, crease_cos)
    rc, h = _create(capi, v, f, crease_cos)
    assert rc == 0, _err(capi)
    try:
        ne, ns, nb = C.c_int64(), C.c_int64(), C.c_int64()
        assert capi.lib().fdcm_mesh_info(h, C.byref(ne), C.byref(ns), C.byref(nb)) == 0
        assert (ne.value, ns.value, nb.value) == (len(ref.everts), int(ref.sharp.sum()), int((ref.efaces[:, 1] < 0).sum()))
        verts, faces = np.full((ne.value, 2), -9, dtype=np.int32), np.full((ne.value, 2), -9, dtype=np.int32)
        sharp = np.full(ne.value, 9, dtype=np.uint8)
        assert capi.lib().fdcm_mesh_edges(h, verts.ctypes.data_as(I32P), faces.ctypes.data_as(I32P), sharp.ctypes.data_as(U8P)) == 0
        assert np.array_equal(verts, ref.everts) and np.array_equal(faces, ref.efaces) and np.array_equal(sharp, ref.sharp)
        assert capi.lib().fdcm_mesh_edges(h, None, None, None) == 0
    finally:
        capi.lib().fdcm_mesh_free(h)
    if crease_cos == -1.0:
        assert int(ref.sharp.sum()) == int(((ref.efaces[:, 1] < 0) | (ref.sharp == 1)).sum())


def test_python_mesh(capi):
    import openfdcm_amd as O
    m = O.Mesh(V, F)
    assert (m.n_edges, m.n_sharp, m.n_boundary) == (18, 12, 0)
    verts, faces, sharp = m.edges()
    assert verts.shape == (18, 2) and faces.shape == (18, 2) and sharp.sum() == 12 and np.all(verts[:, 0] < verts[:, 1])
    assert m.default_depth_tolerance() == MR.default_depth_tol(V) == np.float32(1e-4 * np.sqrt(3.0))
    assert O.Mesh(V, F, crease_angle=np.deg2rad(91)).n_sharp == 0
    m.close()
    m.close()
    with pytest.raises(O._capi.FdcmError, match="non-manifold"):
        O.Mesh(*MC.non_manifold())
    with pytest.raises(ValueError):
        O.Mesh(V.reshape(-1), F)
    with pytest.raises(ValueError):
        O.templates_from_mesh(O.Mesh(V, F), np.zeros((2, 2)), 10.0)


@pytest.mark.parametrize("n,hemisphere", [(1, True), (24, True), (25, False), (1000, True), (1000, False)])
def test_view_rotations(n, hemisphere):
    import openfdcm_amd as O
    R = O.view_rotations(n, hemisphere)
    assert R.shape == (n, 3, 3) and R.dtype == np.float32
    R64 = R.astype(np.float64)
    assert np.abs(R64 @ R64.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-6
    assert np.abs(np.linalg.det(R64) - 1.0).max() <= 1e-6
    # the documented direction row: the Fibonacci spiral, and R turns it onto +Z
    k = np.arange(n)
    z = 1.0 - (k + 0.5) / n if hemisphere else 1.0 - (2.0 * k + 1.0) / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    d = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], axis=1)
    assert np.abs(R64[:, 2, :] - d).max() <= 1e-6
    assert np.abs(np.einsum("nij,nj->ni", R64, d) - [0, 0, 1]).max() <= 1e-6
    # the in-plane rule: the first row is horizontal and at right angles to d
    assert np.abs(R64[:, 0, 2]).max() == 0 and np.abs(np.einsum("ni,ni->n", R64[:, 0, :], d)).max() <= 1e-6
    assert (z > 0).all() if hemisphere else (z.min() < -0.9)
    if n >= 24:    # no two views alike
        g = R64[:, 2, :] @ R64[:, 2, :].T
        assert (g - 2 * np.eye(n)).max() < 1 - 1e-4
    with pytest.raises(ValueError):
        O.view_rotations(0)


def test_record_rotations():
    import openfdcm_amd as O
    views = O.view_rotations(5)
    rec = np.zeros(3, dtype=O._capi.MATCH_DTYPE)
    c, s = np.float32(np.cos(np.deg2rad(30))), np.float32(np.sin(np.deg2rad(30)))
    rec["tmpl_idx"] = [4, 0, 2]
    rec["transform"][0] = [c, -s, 11.5, s, c, -7.25]
    rec["transform"][1] = [1, 0, 0, 0, 1, 0]
    rec["transform"][2] = [0, -1, 3, 1, 0, 4]
    rot, pos = O.record_rotations(rec, views)
    assert rot.shape == (3, 3, 3) and rot.dtype == np.float64 and pos.tolist() == [[11.5, -7.25], [0, 0], [3, 4]]
    rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)
    assert np.array_equal(rot[0], rz @ views[4].astype(np.float64)) and np.array_equal(rot[1], views[0].astype(np.float64))
    assert np.array_equal(rot[2], np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]]) @ views[2].astype(np.float64))
    assert np.abs(rot[0] - MC.rot("z", 30.0) @ views[4].astype(np.float64)).max() <= 1e-6
    # a MatchList and a list of Match do as well
    assert np.array_equal(O.record_rotations(O.MatchList(rec), views)[0], rot)
    with pytest.raises(ValueError):
        O.record_rotations(rec, views[:4])
    rot, pos = O.record_rotations(rec[:0], views)
    assert rot.shape == (0, 3, 3) and pos.shape == (0, 2)
