"""CPU-only checks of the pinhole entry points of the C ABI (include/fdcm.h, "Templates from a mesh: pinhole views"): every
argument error is FDCM_EINVAL with a message before any device work, and a refused call writes nothing.  No call here reaches a
GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_cases as MC

EINVAL = -1
I32P, U64P, I64P = C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


@pytest.fixture(scope="module")
def cube(capi):
    v, f = MC.cube()
    h = C.c_void_p()
    assert capi.lib().fdcm_mesh_create(capi.fptr(v), len(v), f.ctypes.data_as(I32P), len(f), MC.COS30, C.byref(h)) == 0
    yield h
    assert capi.lib().fdcm_mesh_free(h) == 0


FAR = np.float32([0, 0, -6])


def _lines(capi, mesh, views=MC.IDENTITY, positions=FAR, n_views=1, camera=(100.0, 0.1), params=(0.0, 2.0, 0, -1.0), lines=True,
           offsets=True):
    out, off = C.POINTER(C.c_float)(), np.full(max(n_views, 0) + 1, -7, dtype=np.int64)
    cam = None if camera is None else C.byref(capi.MeshCamera(*camera))
    par = None if params is None else C.byref(capi.MeshLineParams(*params))
    rc = capi.lib().fdcm_mesh_view_lines_cam(mesh, None if views is None else capi.fptr(views), None if positions is None else capi.fptr(positions),
                                             n_views, cam, par, C.byref(out) if lines else None, off.ctypes.data_as(I64P) if offsets else None)
    assert not out
    return rc, off


def _two(bad):
    return np.stack([FAR, np.float32(bad)])


ERRORS = [
    (dict(mesh=None), "mesh is null"), (dict(views=None), "views is null"), (dict(positions=None), "positions is null"),
    (dict(camera=None), "camera is null"), (dict(params=None), "params is null"), (dict(lines=False), "lines_out is null"),
    (dict(offsets=False), "offsets_out is null"), (dict(n_views=-1), "n_views"), (dict(n_views=65537), "n_views"),
    (dict(camera=(0.0, 0.1)), "focal"), (dict(camera=(-5.0, 0.1)), "focal"), (dict(camera=(INF, 0.1)), "focal"), (dict(camera=(NAN, 0.1)), "focal"),
    (dict(camera=(100.0, 0.0)), "near"), (dict(camera=(100.0, -1.0)), "near"), (dict(camera=(100.0, INF)), "near"), (dict(camera=(100.0, NAN)), "near"),
    (dict(views=np.stack([MC.IDENTITY] * 2), n_views=2, positions=_two([0, 0, 0.0])), "position 1 is not in front"),
    (dict(views=np.stack([MC.IDENTITY] * 2), n_views=2, positions=_two([0, 0, 2.0])), "position 1 is not in front"),
    (dict(views=np.stack([MC.IDENTITY] * 2), n_views=2, positions=_two([NAN, 0, -6.0])), "position 1 has an entry that is not finite"),
    (dict(views=np.stack([MC.IDENTITY] * 2), n_views=2, positions=_two([0, INF, -6.0])), "position 1 has an entry that is not finite"),
    (dict(views=np.stack([MC.IDENTITY] * 2), n_views=2, positions=_two([0, 0, -INF])), "position 1 has an entry that is not finite"),
    (dict(views=np.stack([MC.IDENTITY, np.where(np.eye(3) == 1, np.float32("nan"), MC.GENERIC)]).astype(np.float32), n_views=2,
          positions=_two(FAR)), "view 1 has an entry that is not finite"),
    (dict(params=(-1e-6, 2.0, 0, -1.0)), "depth_tol"), (dict(params=(NAN, 2.0, 0, -1.0)), "depth_tol"),
    (dict(params=(0.0, -1.0, 0, -1.0)), "min_length"), (dict(params=(0.0, INF, 0, -1.0)), "min_length"),
    (dict(params=(0.0, 2.0, 2, -1.0)), "visibility"), (dict(params=(0.0, 2.0, 0, NAN)), "join_tolerance"),
    (dict(params=(0.0, 2.0, 1, INF)), "join_tolerance"),
]


@pytest.mark.parametrize("kw,what", ERRORS, ids=lambda v: str(v)[:60])
def test_view_lines_cam_argument_errors(capi, cube, kw, what):
    kw = dict(kw)
    rc, off = _lines(capi, kw.pop("mesh", cube), **kw)
    assert rc == EINVAL and what in capi.lib().fdcm_last_error().decode(), capi.lib().fdcm_last_error().decode()
    assert np.all(off == -7)      # a refused call writes nothing


def test_zero_views_are_no_lines_and_no_device(capi, cube):
    rc, off = _lines(capi, cube, n_views=0)
    assert rc == 0 and off.tolist() == [0]
    rc, off = _lines(capi, cube, views=None, positions=None, n_views=0)
    assert rc == 0 and off.tolist() == [0]


def test_view_items_cam_argument_errors(capi, cube):
    lib = capi.lib()
    box, keys = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.uint64)
    view, pos = capi.fptr(MC.IDENTITY), capi.fptr(FAR)
    cam = C.byref(capi.MeshCamera(100.0, 0.1))
    b, k = box.ctypes.data_as(I32P), keys.ctypes.data_as(U64P)
    for args, what in (((None, view, pos, cam, b, k, 4), "mesh is null"), ((cube, None, pos, cam, b, k, 4), "view is null"),
                       ((cube, view, None, cam, b, k, 4), "position is null"), ((cube, view, pos, None, b, k, 4), "camera is null"),
                       ((cube, view, pos, cam, None, k, 4), "box_out is null"), ((cube, view, pos, cam, b, k, -1), "capacity"),
                       ((cube, view, pos, C.byref(capi.MeshCamera(0.0, 0.1)), b, k, 4), "focal"),
                       ((cube, view, pos, C.byref(capi.MeshCamera(100.0, 0.0)), b, k, 4), "near"),
                       ((cube, view, capi.fptr(np.float32([0, 0, 1])), cam, b, k, 4), "position 0 is not in front")):
        assert lib.fdcm_mesh_view_items_cam(*args) == EINVAL and what in lib.fdcm_last_error().decode(), (what, lib.fdcm_last_error().decode())
    assert not box.any() and not keys.any()


def test_structs_and_table(capi):
    assert C.sizeof(capi.MeshCamera) == 8 and [n for n, _ in capi.MeshCamera._fields_] == ["focal", "near"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fdcm.h")).read()
    for name in ("fdcm_mesh_view_lines_cam", "fdcm_mesh_view_items_cam"):
        assert f"int {name}(" in header and hasattr(capi.lib(), name)
    assert "typedef struct { float focal, near; } fdcm_mesh_camera;" in header
