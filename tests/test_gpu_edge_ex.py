"""Edges with smoothing, hysteresis and a minimum chain length on the GPU (include/fdcm.h) against tests/edge_ex_ref.py: label
images over the sizes that matter to the 64 x 16 tile, the serpentines, an edge that leaves its tiles diagonally, the identity with
the single-threshold kernel, volumes, rebuilds on one handle, device input and the blank image.  Every comparison is on bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

import edge_ex_ref as X
import edge_ref
from helpers import EDGE_SCENES
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FMAX = edge_ref.FMAX
# exact fit of the tile, one pixel over, smaller than the halo, one tile wide and many tall, components across many tile borders
SIZES = [(1, 1), (4, 1), (5, 3), (64, 16), (65, 17), (48, 40), (97, 61), (61, 97), (130, 200), (700, 9), (12, 2100)]
PARAMS = [(20, 60, 1), (20, 60, 8), (30, 100, 1), (60, 60, 1), (1, 1442, 1)]   # (low, high, min_pixels)
DEPTHS = (1, 6, 30, 180)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def image(width, height, seed=None):
    img = edge_ref.synthetic_image(width, height, width * 1000 + height if seed is None else seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def serpentine(width, height, ramp=True):
    img = X.serpentine(width, height, ramp)
    img.setflags(write=False)
    return img


def strided(img, extra=3):
    buf = np.full((img.shape[0], img.shape[1] + extra), 0xA5, dtype=np.uint8)
    buf[:, :img.shape[1]] = img
    return buf[:, :img.shape[1]]


class Referee:
    """The referee's answers for one image and one smoothing, computed once: the edge set per (low, high, min_pixels), and per
    depth the labels of every pixel that passes thinning at low = 1, of which every edge set is a subset."""

    def __init__(self, img, smooth):
        self.img, self.smooth = img, smooth
        self.all, _, self.gx, self.gy = X.candidates(img, smooth, 1, 1)
        self.by_depth, self.masks = {}, {}

    def labels(self, depth, low, high, min_pixels):
        if depth not in self.by_depth:
            self.by_depth[depth] = X.labels_of(self.all, self.gx, self.gy, depth)
        key = (low, high, min_pixels)
        if key not in self.masks:
            self.masks[key] = X.edge_mask(self.img, self.smooth, low, high, min_pixels)[0]
            assert not (self.masks[key] & ~self.all).any()
        return np.where(self.masks[key], self.by_depth[depth], np.uint8(255)).astype(np.uint8)


_referees = {}


def referee(img, smooth):
    key = (img.shape, img.tobytes(), smooth)
    if key not in _referees:
        _referees[key] = Referee(img, smooth)
    return _referees[key]


def ex_labels(img, depth, smooth, low, high, min_pixels):
    """fdcm_edge_labels_ex itself: the Python keywords would route smooth = 0, low = None, min_pixels = 1 to the old call."""
    from openfdcm_amd import _capi
    from openfdcm_amd.engine import _pixels
    p, w, h, stride, _, keep = _pixels(img, "image")
    out = np.empty((h, w), dtype=np.uint8)
    e = _capi.EdgeParams(smooth, low, high, min_pixels)
    _capi.check(_capi.lib().fdcm_edge_labels_ex(p, w, h, stride, depth, C.byref(e), C.c_void_p(out.ctypes.data)))
    return out


# ---------------------------------------------------------------- labels
def test_the_referee_shortcut_is_the_referee():
    img = image(48, 40, 1)
    for smooth in (0, 1, 2):
        assert np.array_equal(referee(img, smooth).labels(30, 20, 60, 8), X.edge_labels(img, 30, smooth, 20, 60, 8))


@pytest.mark.parametrize("smooth", [0, 1, 2])
@pytest.mark.parametrize("width,height", SIZES, ids=lambda v: str(v))
def test_edge_labels_equal_the_definition(width, height, smooth):
    import openfdcm_amd
    img = image(width, height)
    ref = referee(img, smooth)
    views = [("packed", img), ("stride+3", strided(img))]
    assert views[1][1].strides[0] == width + 3
    for (low, high, min_pixels) in PARAMS:
        for depth in DEPTHS:
            want = ref.labels(depth, low, high, min_pixels)
            for name, view in views:
                got = openfdcm_amd.edge_labels(view, depth=depth, threshold=high, low=low, smooth=smooth, min_pixels=min_pixels)
                assert got.dtype == np.uint8 and got.shape == (height, width)
                assert np.array_equal(got, want), (name, low, high, min_pixels, depth, np.argwhere(got != want)[:5])


@pytest.mark.parametrize("smooth", [0, 1])
@pytest.mark.parametrize("width,height,ramp", [(130, 200, True), (200, 130, True), (130, 200, False)], ids=lambda v: str(v))
def test_serpentines(width, height, ramp, smooth):
    import openfdcm_amd
    img = serpentine(width, height, ramp)
    want = referee(img, smooth).labels(30, 20, 100, 1)
    n = int((want != 255).sum())
    assert n == ({130: 5900, 200: 5786}[width] if ramp else 0)
    for view in (img, strided(img)):
        got = openfdcm_amd.edge_labels(view, depth=30, threshold=100, low=20, smooth=smooth)
        assert np.array_equal(got, want), (int((got != 255).sum()), n)


def diagonal_step(width, height, mirrored):
    """70 left of and on the line x = y, max(80, 130 - 2 y) right of it: one edge that leaves every tile it crosses through a
    corner or a side, strong only where the step is high, in the first rows."""
    y, x = np.mgrid[0:height, 0:width]
    img = np.where(x <= y, 70, np.maximum(80, 130 - 2 * y)).astype(np.uint8)
    return np.ascontiguousarray(img[:, ::-1]) if mirrored else img


@pytest.mark.parametrize("smooth", [0, 1])
@pytest.mark.parametrize("mirrored", [False, True], ids=["diagonal", "mirrored"])
@pytest.mark.parametrize("width,height", [(130, 200), (200, 200)], ids=lambda v: str(v))
def test_diagonal_edge_across_tile_corners(width, height, mirrored, smooth):
    """The whole chain hangs on strong pixels in one corner of the image, through links that cross tile borders diagonally."""
    import openfdcm_amd
    img = diagonal_step(width, height, mirrored)
    edge, cand, strong, gx, gy = X.edge_mask(img, smooth, 20, 100, 1)
    ys, xs = np.nonzero(edge)
    assert X.components(cand)[1] == 1 and np.array_equal(edge, cand)          # one chain, kept whole
    assert len(ys) == {130: (257, 258), 200: (397, 398)}[width][smooth]
    assert len(set(zip(ys // 16, xs // 64))) == {130: 11, 200: 16}[width]     # the 64 x 16 tiles it crosses
    sy, sx = np.nonzero(strong)
    assert len(sy) > 0 and sy.max() < 32 and ys.max() >= min(width, height) - 2  # strong in the first two tile rows only
    assert (sx.min() >= width - 64) if mirrored else (sx.max() < 64)
    want = X.labels_of(edge, gx, gy, 30)
    for view in (img, strided(img)):
        got = openfdcm_amd.edge_labels(view, depth=30, threshold=100, low=20, smooth=smooth, min_pixels=1)
        assert np.array_equal(got, want), (int((got != 255).sum()), len(ys), np.argwhere(got != want)[:5])


@pytest.mark.parametrize("width,height", [(48, 40), (97, 61), (130, 200), (700, 9)], ids=lambda v: str(v))
def test_one_threshold_through_ex_is_the_existing_kernel(width, height):
    import openfdcm_amd
    img = image(width, height)
    for t in (1, 20, 60, 1442):
        for depth in (6, 30):
            old = openfdcm_amd.edge_labels(img, depth=depth, threshold=t)
            assert np.array_equal(ex_labels(img, depth, 0, t, t, 1), old), (t, depth)
            assert np.array_equal(openfdcm_amd.edge_labels(img, depth=depth, threshold=t, low=t), old)


# ---------------------------------------------------------------- volumes
OPTS = dict(low=20, smooth=1, min_pixels=8)


def want_labels(img, depth):
    return referee(img, 1).labels(depth, 20, 60, 8)


@pytest.mark.parametrize("distance", [O.L2, O.L2_SQUARED, O.L1], ids=["L2", "L2sq", "L1"])
@pytest.mark.parametrize("border", [0, 3])
@pytest.mark.parametrize("depth", [6, 30])
@pytest.mark.parametrize("name", ["48x40", "97x61", "130x200", "serpentine"])
def test_volume_is_that_of_the_referees_labels(name, depth, border, distance):
    from openfdcm_amd.engine import DeviceFeatureMap
    img = {"48x40": image(48, 40, 1), "97x61": image(97, 61, 2), "130x200": image(130, 200), "serpentine": serpentine(130, 200)}[name]
    lab = want_labels(img, depth)
    assert (lab != 255).any()
    a = DeviceFeatureMap.build_image(img, 60, border=border, depth=depth, coeff=5.0, distance=distance, **OPTS)
    b = DeviceFeatureMap.build_labels(lab, border=border, depth=depth, coeff=5.0, distance=distance)
    va = a.volume()
    assert (a.width, a.height) == (img.shape[1] + 2 * border, img.shape[0] + 2 * border)
    assert np.array_equal(a.scene_translation, np.float32([border, border])) and np.array_equal(a.keys, b.keys)
    assert same_bits(va, b.volume())
    if name == "48x40":
        assert same_bits(va, edge_ref.reference_volume(lab, border, depth, 5.0, distance)[1])
    a.close(); b.close()


# ---------------------------------------------------------------- rebuilds
def _order_counts():
    from openfdcm_amd import _capi
    h, p = C.c_int64(), C.c_int64()
    _capi.check(_capi.lib().fdcm_selftest_sweep_order_counts(C.byref(h), C.byref(p)))
    return h.value, p.value


def test_one_handle_rebuilt_with_and_without_options_and_from_lines():
    from openfdcm_amd.engine import DeviceFeatureMap
    A, B = image(97, 61, 2), image(48, 40, 1)
    scene, _, _, _ = EDGE_SCENES["offset"]
    depth, coeff = 12, 5.0
    kw = dict(depth=depth, coeff=coeff, distance=O.L2)
    other = dict(low=30, smooth=2, min_pixels=3)
    fresh = {
        "a_opts": DeviceFeatureMap.build_image(A, 60, border=1, **kw, **OPTS),
        "lines": DeviceFeatureMap.build(scene, padding=0.0, **kw),
        "a_plain": DeviceFeatureMap.build_image(A, 60, border=1, **kw),
        "b_other": DeviceFeatureMap.build_image(B, 100, border=0, **kw, **other),
    }
    vols = {k: f.volume() for k, f in fresh.items()}
    assert same_bits(vols["a_opts"], edge_ref.reference_volume(want_labels(A, depth), 1, depth, coeff, O.L2)[1])
    assert same_bits(vols["b_other"], edge_ref.reference_volume(referee(B, 2).labels(depth, 30, 100, 3), 0, depth, coeff, O.L2)[1])
    assert not same_bits(vols["a_opts"], vols["a_plain"])
    fm = DeviceFeatureMap.build_image(B, 60, border=0, **kw)              # a handle that has never held the new scratch
    fm.rebuild_image(A, 60, border=1, **OPTS)
    assert (fm.width, fm.height) == (99, 63) and same_bits(fm.volume(), vols["a_opts"])
    fm.rebuild(scene)
    assert same_bits(fm.volume(), vols["lines"]) and np.array_equal(fm.scene_translation, fresh["lines"].scene_translation)
    fm.rebuild_image(A, 60, border=1)
    assert same_bits(fm.volume(), vols["a_plain"])
    fm.rebuild_image(B, 100, border=0, **other)
    assert (fm.width, fm.height) == (48, 40) and same_bits(fm.volume(), vols["b_other"])
    # a rebuild's parameter errors leave the handle as it was
    from openfdcm_amd import _capi
    for bad in (dict(low=0), dict(low=101), dict(smooth=3), dict(min_pixels=0)):
        with pytest.raises(_capi.FdcmError):
            fm.rebuild_image(B, 100, **bad)
    assert same_bits(fm.volume(), vols["b_other"])
    p = C.c_void_p(B.ctypes.data)
    assert _capi.lib().fdcm_featuremap_rebuild_image_ex(fm._h, p, 48, 40, 48, 0, None, 0) == -1
    assert "params is null" in _capi.lib().fdcm_last_error().decode()
    for f in list(fresh.values()) + [fm]:
        f.close()


def test_first_build_of_a_shape_orders_the_sweep_by_the_device_proxy():
    """As tests/test_gpu_image_featuremap.py's: 30 x 18 (slice, chunk) pairs want a launch order; the first build with options
    counts the proxy on the device behind the edge kernels, the next build of the shape takes the sweep's history."""
    from openfdcm_amd.engine import DeviceFeatureMap
    a, b = image(20, 1100, 5), image(20, 1100, 6)
    h0, p0 = _order_counts()
    fm = DeviceFeatureMap.build_image(a, 60, depth=30, distance=O.L2_SQUARED, **OPTS)
    h1, p1 = _order_counts()
    assert (h1 - h0, p1 - p0) == (0, 1)
    assert same_bits(fm.volume(), edge_ref.reference_volume(want_labels(a, 30), 0, 30, 5.0, O.L2_SQUARED)[1])
    fm.rebuild_image(b, 60, **OPTS)
    h2, p2 = _order_counts()
    assert (h2 - h1, p2 - p1) == (1, 0)
    assert same_bits(fm.volume(), edge_ref.reference_volume(want_labels(b, 30), 0, 30, 5.0, O.L2_SQUARED)[1])
    fm.close()


# ---------------------------------------------------------------- device input, downstream
def _templates():
    box = lambda x0, y0, x1, y1: np.array([[x0, y0, x1, y0], [x1, y0, x1, y1], [x1, y1, x0, y1], [x0, y1, x0, y0]], dtype=np.float32).T
    return [box(0, 0, 20, 12), box(2, 1, 11, 30), np.array([[0, 0, 14, 9], [14, 9, 3, 17], [3, 17, 0, 0]], dtype=np.float32).T]


def test_device_tensors_through_build_image_featuremap():
    import torch

    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap
    img = image(97, 61, 2)
    params = fd.Dt3CpuParameters(depth=6, dt3Coeff=5.0, distance=fd.L2)
    lab = referee(img, 1).labels(6, 20, 60, 1)
    ref = DeviceFeatureMap.build_labels(lab, border=0, depth=6, coeff=5.0, distance=O.L2)
    want_vol = ref.volume()
    tmpls = _templates()
    want = fd.records_of(fd.exhaustive_search(ref, tmpls, k=8))
    assert len(want) == 24
    t = torch.from_numpy(np.array(img)).cuda()
    wide = torch.full((61, 100), 0xA5, dtype=torch.uint8, device="cuda")   # rows 3 bytes longer, read in place
    wide[:, :97] = t
    fd.clear_featuremap_pool()
    for frame in (t, wide[:, :97], t):                                      # a fresh handle, then the pool's, rebuilt
        dt3 = fd.build_image_featuremap(frame, params, threshold=60, low=20, smooth=1)
        assert same_bits(dt3._fm.volume(), want_vol)
        got = fd.records_of(fd.exhaustive_search(dt3, tmpls, k=8))
        assert got.tobytes() == want.tobytes()
        del dt3
    fd.clear_featuremap_pool()
    ref.close()


def test_blank_image_gives_flt_max_not_an_error():
    """No edge pixel: every slice of stage 1 is FLT_MAX throughout, and the volume is what the later stages make of that (the
    reference volume of a label image without labels, which is also the plain build's)."""
    import openfdcm_amd
    from openfdcm_amd.engine import DeviceFeatureMap
    blank = np.full((40, 48), 90, dtype=np.uint8)
    none = np.full((40, 48), 255, dtype=np.uint8)
    assert (edge_ref.reference_volume(none, 2, 6, 5.0, O.L2_SQUARED, 1)[1] == FMAX).all()
    want = edge_ref.reference_volume(none, 2, 6, 5.0, O.L2_SQUARED)[1]
    plain = DeviceFeatureMap.build_image(blank, 60, border=2, depth=6, coeff=5.0, distance=O.L2_SQUARED)
    assert same_bits(plain.volume(), want)
    plain.close()
    for opts in (dict(low=20, smooth=1, min_pixels=8), dict(low=1, smooth=0, min_pixels=1), dict(low=60, smooth=2, min_pixels=100)):
        assert (openfdcm_amd.edge_labels(blank, depth=6, threshold=60, **opts) == 255).all()
        fm = DeviceFeatureMap.build_image(blank, 60, border=2, depth=6, coeff=5.0, distance=O.L2_SQUARED, **opts)
        vol = fm.volume()
        assert vol.shape == (6, 52, 44) and same_bits(vol, want)
        fm.close()
    # an image with candidates and no strong pixel is blank too
    img = serpentine(130, 200, False)
    fm = DeviceFeatureMap.build_image(img, 100, depth=6, coeff=5.0, distance=O.L2_SQUARED, low=20)
    assert same_bits(fm.volume(), edge_ref.reference_volume(np.full((200, 130), 255, dtype=np.uint8), 0, 6, 5.0, O.L2_SQUARED)[1])
    fm.close()
