"""CPU-only checks of the exhaustive translation search's C ABI (include/fdcm.h, "exhaustive translation search"): the
library exports its entry points, and the argument checks that come before any device work return FDCM_EINVAL with a
message.  No GPU compute: every call here fails its checks before it touches a handle."""
import ctypes as C
import os

import pytest

EINVAL = -1
NEW_SYMBOLS = ["fdcm_exhaustive_window", "fdcm_search_exhaustive", "fdcm_score_map", "fdcm_score_map_device"]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    return _capi


def _err(capi):
    return capi.lib().fdcm_last_error().decode()


def test_exports_the_exhaustive_entry_points(capi):
    lib = C.CDLL(capi.LIB_PATH)
    bound = {s[0] for s in capi.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in bound, name
    assert C.sizeof(capi.Grid) == 24


def test_null_pointers_are_einval(capi):
    lib = capi.lib()
    g = capi.Grid(0, 0, 4, 4, 1, 1)
    out, n = C.c_void_p(), C.c_int64()
    assert lib.fdcm_search_exhaustive(None, None, C.byref(g), 1, 0, C.byref(out), C.byref(n)) == EINVAL
    assert "null" in _err(capi)
    assert lib.fdcm_search_exhaustive(None, None, None, 1, 0, C.byref(out), C.byref(n)) == EINVAL
    assert "grid is null" in _err(capi)
    assert lib.fdcm_score_map(None, None, C.byref(g), None) == EINVAL
    assert "null" in _err(capi)
    assert lib.fdcm_score_map_device(None, None, C.byref(g), None) == EINVAL
    assert "null" in _err(capi)
    assert lib.fdcm_exhaustive_window(None, None, 1, 1, C.byref(capi.Grid())) == EINVAL
    assert "null" in _err(capi)


@pytest.mark.parametrize("grid,what", [
    ((0, 0, 4, 4, 0, 1), "stride"), ((0, 0, 4, 4, 1, 0), "stride"), ((0, 0, 4, 4, -3, 2), "stride"),
    ((0, 0, 0, 4, 1, 1), "nx and ny"), ((0, 0, 4, -1, 1, 1), "nx and ny"),
    ((0, 0, 1 << 16, 1 << 15, 1, 1), "2^31"), ((0, 0, 0x7fffffff, 2, 1, 1), "2^31"),
])
def test_bad_grids_are_einval(capi, grid, what):
    lib = capi.lib()
    g = capi.Grid(*grid)
    out, n = C.c_void_p(), C.c_int64()
    assert lib.fdcm_search_exhaustive(None, None, C.byref(g), 1, 0, C.byref(out), C.byref(n)) == EINVAL
    assert what in _err(capi)
    assert lib.fdcm_score_map(None, None, C.byref(g), None) == EINVAL
    assert what in _err(capi)
    assert lib.fdcm_score_map_device(None, None, C.byref(g), None) == EINVAL
    assert what in _err(capi)


@pytest.mark.parametrize("k", [0, -1, 65, 1000])
def test_k_out_of_range_is_einval(capi, k):
    g = capi.Grid(0, 0, 4, 4, 1, 1)
    out, n = C.c_void_p(), C.c_int64()
    assert capi.lib().fdcm_search_exhaustive(None, None, C.byref(g), k, 0, C.byref(out), C.byref(n)) == EINVAL
    assert "k must be in [1, 64]" in _err(capi)


@pytest.mark.parametrize("sx,sy", [(0, 1), (1, 0), (-2, 5)])
def test_window_stride_is_checked_first(capi, sx, sy):
    assert capi.lib().fdcm_exhaustive_window(None, None, sx, sy, C.byref(capi.Grid())) == EINVAL
    assert "stride" in _err(capi)
