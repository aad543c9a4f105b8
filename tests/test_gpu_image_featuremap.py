"""Feature maps from images on the GPU (include/fdcm.h, "feature maps from images") against tests/edge_ref.py: the label
image, the volume stage by stage, the labels and device-memory entries, rebuilds across seed sources, and everything
downstream of an image-built map.  Every comparison is on bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

import edge_ref
from helpers import EDGE_SCENES
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FMAX = edge_ref.FMAX


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def image(width, height, seed=None):
    img = edge_ref.synthetic_image(width, height, width * 1000 + height if seed is None else seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def ref_labels(width, height, depth, threshold=60, seed=None):
    lab = edge_ref.edge_labels(image(width, height, seed), depth, threshold)
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def ref_volume(width, height, depth, border, distance, stop_after, seed=None):
    keys, vol = edge_ref.reference_volume(ref_labels(width, height, depth, 60, seed), border, depth, 5.0, distance, stop_after)
    vol.setflags(write=False)
    return keys, vol


def strided(img, extra=3):
    """The same pixels in rows `extra` bytes longer, filled with a value no pixel may be taken from."""
    buf = np.full((img.shape[0], img.shape[1] + extra), 0xA5, dtype=np.uint8)
    buf[:, :img.shape[1]] = img
    return buf[:, :img.shape[1]]


# ---------------------------------------------------------------- the test images (computed here with edge_ref's rule)
def test_the_test_images_have_edges_in_every_bin():
    small, big = ref_labels(48, 40, 6, 60, 1), ref_labels(97, 61, 30, 60, 2)
    assert set(np.unique(small)) == set(range(6)) | {255} and (small != 255).sum() >= 100
    assert set(np.unique(big)) == set(range(30)) | {255} and (big != 255).sum() >= 200
    assert (edge_ref.edge_labels(np.full((40, 48), 90, dtype=np.uint8), 6, 1) == 255).all()


# ---------------------------------------------------------------- labels
SIZES = [(1, 1), (4, 1), (5, 3), (48, 40), (97, 61), (61, 97), (64, 64), (130, 200)]


@pytest.mark.parametrize("width,height", SIZES, ids=lambda v: str(v))
def test_edge_labels_equal_the_definition(width, height):
    import openfdcm_amd
    img = image(width, height)
    views = [("packed", img), ("stride+3", strided(img))]
    assert views[1][1].strides[0] == width + 3
    for threshold in (1, 60, 1442):
        for depth in (1, 6, 7, 30, 180):
            want = edge_ref.edge_labels(img, depth, threshold)
            for name, view in views:
                got = openfdcm_amd.edge_labels(view, depth=depth, threshold=threshold)
                assert got.dtype == np.uint8 and got.shape == (height, width)
                assert np.array_equal(got, want), (name, threshold, depth, np.argwhere(got != want)[:5])


def test_edge_labels_of_a_saturated_step_at_the_last_threshold():
    import openfdcm_amd
    img = np.zeros((12, 70), dtype=np.uint8)
    img[5:, 33:] = 255                                           # a corner: m2 up to 2 * 1020^2 at most, 1442^2 is below that
    for thr in (1020, 1442):
        want = edge_ref.edge_labels(img, 30, thr)
        assert np.array_equal(openfdcm_amd.edge_labels(img, depth=30, threshold=thr), want)
    assert (edge_ref.edge_labels(img, 30, 1020) != 255).any()


# ---------------------------------------------------------------- the volume, stage by stage
def build_image(img, depth, border, distance, stop_after):
    from openfdcm_amd.engine import DeviceFeatureMap
    return DeviceFeatureMap.build_image(img, 60, border=border, depth=depth, coeff=5.0, distance=distance, stop_after=stop_after)


def check_stages(width, height, depth, border, distance, seed=None, img=None):
    img = image(width, height, seed) if img is None else img
    for stop in (1, 2, 3):
        fm = build_image(img, depth, border, distance, stop)
        keys, want = ref_volume(width, height, depth, border, distance, stop, seed)
        assert (fm.width, fm.height, fm.depth) == (width + 2 * border, height + 2 * border, len(keys))
        assert np.array_equal(fm.scene_translation, np.float32([border, border])) and np.array_equal(fm.keys, keys)
        got = fm.volume()
        assert same_bits(got, want), (stop, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5])
        if stop == 1:   # the zeros of the transforms are exactly the labelled pixels, shifted by the border
            lab = ref_labels(width, height, depth, 60, seed)
            for k in range(len(keys)):
                z = np.zeros((fm.width, fm.height), dtype=bool)
                ys, xs = np.nonzero(lab == k)
                z[xs + border, ys + border] = True
                assert np.array_equal(got[k] == 0, z), k
        fm.close()


@pytest.mark.parametrize("distance", [O.L2_SQUARED, O.L2, O.L1], ids=["L2sq", "L2", "L1"])
@pytest.mark.parametrize("border", [0, 3])
@pytest.mark.parametrize("width,height,depth", [(w, h, d) for (w, h) in [(48, 40), (97, 61), (61, 97), (130, 200)] for d in (6, 30)],
                         ids=lambda v: str(v))
def test_volume_stage_by_stage(width, height, depth, border, distance):
    check_stages(width, height, depth, border, distance)


@pytest.mark.parametrize("distance", [O.L2_SQUARED, O.L2, O.L1], ids=["L2sq", "L2", "L1"])
@pytest.mark.parametrize("width,height,border", [(20, 1100, 0), (20, 1100, 3), (12, 2100, 0), (12, 2100, 3)], ids=lambda v: str(v))
def test_tall_maps_take_the_other_descriptor_shapes(width, height, border, distance):
    """17 and 33 chunks of 64 rows per column: the <32, 64> and <64, 32> shapes of the tile kernel (the small maps take <16, 64>)."""
    assert (height + 63) // 64 in (18, 33)
    check_stages(width, height, 2, border, distance)


def test_a_wide_map():
    check_stages(700, 9, 6, 1, O.L2_SQUARED)


def test_blank_image_and_single_slice_image():
    blank = np.full((40, 48), 90, dtype=np.uint8)
    step = np.full((40, 48), 30, dtype=np.uint8)
    step[:, 20:] = 220                                             # one vertical edge: every seed in slice 0
    assert set(np.unique(edge_ref.edge_labels(step, 6, 60))) == {0, 255}
    for img in (blank, step):
        lab = edge_ref.edge_labels(img, 6, 60)
        for distance in (O.L2_SQUARED, O.L2, O.L1):
            for stop in (1, 2, 3):
                keys, want = edge_ref.reference_volume(lab, 2, 6, 5.0, distance, stop)
                fm = build_image(img, 6, 2, distance, stop)
                assert same_bits(fm.volume(), want), (distance, stop)
                fm.close()
    keys, want = edge_ref.reference_volume(edge_ref.edge_labels(blank, 30, 60), 0, 30, 5.0, O.L2_SQUARED, 1)
    assert (want == FMAX).all()


def test_first_build_orders_the_sweep_by_the_device_proxy_and_the_next_by_history():
    """More (slice, chunk) pairs than the GPU holds workgroups at once (30 x 18 > 2 x 256): the balanced sweep wants a launch
    order, a first build has no history and no line boxes, so pass 1 counts the proxy; the handle's next build of the shape
    takes the costs the sweep left."""
    from openfdcm_amd import _capi
    from openfdcm_amd.engine import DeviceFeatureMap
    counts = lambda: tuple(v.value for v in _counts())

    def _counts():
        h, p = C.c_int64(), C.c_int64()
        _capi.check(_capi.lib().fdcm_selftest_sweep_order_counts(C.byref(h), C.byref(p)))
        return h, p
    h0, p0 = counts()
    a, b = image(20, 1100, 5), image(20, 1100, 6)
    fm = DeviceFeatureMap.build_image(a, 60, depth=30, distance=O.L2_SQUARED, stop_after=1)
    h1, p1 = counts()
    assert (h1 - h0, p1 - p0) == (0, 1)
    assert same_bits(fm.volume(), ref_volume(20, 1100, 30, 0, O.L2_SQUARED, 1, 5)[1])
    fm.rebuild_image(b, 60)
    h2, p2 = counts()
    assert (h2 - h1, p2 - p1) == (1, 0)
    assert same_bits(fm.volume(), ref_volume(20, 1100, 30, 0, O.L2_SQUARED, 3, 6)[1])
    fm.close()


# ---------------------------------------------------------------- labels entry, device input
def test_build_labels_equals_build_image():
    from openfdcm_amd.engine import DeviceFeatureMap
    for (w, h, depth, border) in [(97, 61, 30, 0), (48, 40, 6, 3)]:
        lab = ref_labels(w, h, depth)
        a = build_image(image(w, h), depth, border, O.L2, 3)
        b = DeviceFeatureMap.build_labels(lab, border=border, depth=depth, coeff=5.0, distance=O.L2)
        va = a.volume()
        assert same_bits(va, b.volume()) and np.array_equal(a.scene_translation, b.scene_translation)
        # any value >= m is "no edge"
        other = lab.copy()
        none = np.flatnonzero(other.ravel() == 255)
        other.ravel()[none[::3]] = depth
        other.ravel()[none[1::3]] = 200
        b.rebuild_labels(other, border=border)
        assert same_bits(va, b.volume())
        a.close(); b.close()


def test_device_tensors_give_the_same_volume():
    import torch
    from openfdcm_amd.engine import DeviceFeatureMap
    img = image(97, 61)
    host = build_image(img, 30, 2, O.L2, 3)
    want = host.volume()
    t = torch.from_numpy(np.array(img)).cuda()
    dev = DeviceFeatureMap.build_image(t, 60, border=2, depth=30, coeff=5.0, distance=O.L2)
    assert same_bits(dev.volume(), want)
    wide = torch.full((61, 100), 0xA5, dtype=torch.uint8, device="cuda")   # rows 3 bytes longer, read in place
    wide[:, :97] = t
    dev.rebuild_image(wide[:, :97], 60, border=2)
    assert same_bits(dev.volume(), want)
    lab = torch.from_numpy(np.array(ref_labels(97, 61, 30))).cuda()
    dev.rebuild_labels(lab, border=2)
    assert same_bits(dev.volume(), want)
    host.close(); dev.close()


# ---------------------------------------------------------------- rebuilds across seed sources
def test_one_handle_rebuilt_from_images_and_lines():
    from openfdcm_amd.engine import DeviceFeatureMap
    A, B = image(97, 61), image(48, 40)
    scene, _, _, _ = EDGE_SCENES["offset"]
    depth, coeff = 12, 5.0
    fresh_a = DeviceFeatureMap.build_image(A, 60, border=1, depth=depth, coeff=coeff, distance=O.L2)
    fresh_b = DeviceFeatureMap.build_image(B, 60, border=0, depth=depth, coeff=coeff, distance=O.L2)
    fresh_l = DeviceFeatureMap.build(scene, depth=depth, coeff=coeff, padding=0.0, distance=O.L2)   # an image handle's padding
    va, vb, vl = fresh_a.volume(), fresh_b.volume(), fresh_l.volume()
    assert same_bits(va, edge_ref.reference_volume(edge_ref.edge_labels(A, depth, 60), 1, depth, coeff, O.L2)[1])
    fm = DeviceFeatureMap.build_image(A, 60, border=1, depth=depth, coeff=coeff, distance=O.L2)
    assert same_bits(fm.volume(), va)
    fm.rebuild_image(B, 60, border=0)
    assert (fm.width, fm.height) == (48, 40) and same_bits(fm.volume(), vb)
    fm.rebuild(scene)
    assert (fm.width, fm.height) == (fresh_l.width, fresh_l.height) and same_bits(fm.volume(), vl)
    assert np.array_equal(fm.scene_translation, fresh_l.scene_translation)
    fm.rebuild_image(A, 60, border=1)
    assert (fm.width, fm.height) == (99, 63) and same_bits(fm.volume(), va)
    assert np.array_equal(fm.scene_translation, np.float32([1, 1]))
    # and the reverse: a handle made from lines takes an image
    fresh_l.rebuild_image(B, 60, border=0)
    assert same_bits(fresh_l.volume(), vb)
    for f in (fresh_a, fresh_b, fresh_l, fm):
        f.close()


# ---------------------------------------------------------------- downstream
def _templates():
    box = lambda x0, y0, x1, y1: np.array([[x0, y0, x1, y0], [x1, y0, x1, y1], [x1, y1, x0, y1], [x0, y1, x0, y0]], dtype=np.float32).T
    return [box(0, 0, 20, 12), box(2, 1, 11, 30), np.array([[0, 0, 14, 9], [14, 9, 3, 17], [3, 17, 0, 0]], dtype=np.float32).T]


def test_downstream_calls_take_an_image_map():
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap
    b = 2
    dt3 = fd.build_image_featuremap(image(97, 61), fd.Dt3CpuParameters(depth=6, dt3Coeff=5.0, distance=fd.L2), threshold=60, border=b)
    assert list(dt3.get_feature_size()) == [101, 65] and list(dt3.get_scene_translation()) == [b, b]
    vol = dt3._fm.volume()
    assert same_bits(vol, ref_volume(97, 61, 6, b, O.L2, 3)[1])
    adopted = DeviceFeatureMap.from_volume(dt3._fm.keys, vol, (b, b))
    tmpls = _templates()
    sm, g = fd.score_map(dt3, tmpls)
    sm2, g2 = fd.score_map(adopted, tmpls)
    assert g == g2 and g[2] > 0 and same_bits(sm, sm2) and np.isfinite(sm).any()
    r1 = fd.records_of(fd.exhaustive_search(dt3, tmpls, k=8))
    r2 = fd.records_of(fd.exhaustive_search(adopted, tmpls, k=8))
    assert len(r1) == 24 and r1.tobytes() == r2.tobytes()
    # FeatureMap.evaluate reproduces the records' scores at their translations
    fmap = fd.FeatureMap(dt3)
    for t in range(3):
        rec = r1[r1["tmpl_idx"] == t]
        tr = np.ascontiguousarray(rec["transform"][:, [2, 5]])
        assert same_bits(fmap.evaluate([tmpls[t]], [tr])[0], rec["score"])
    # search() with scene lines of the caller's
    scene = np.array([[10, 8, 40, 8], [40, 8, 40, 30], [15, 50, 60, 42], [70, 10, 88, 44]], dtype=np.float32).T
    got = fd.records_of(fd.search(fd.DefaultMatch(), fd.DefaultSearch(4, 4), fd.BatchOptimize(4), dt3, tmpls, scene))
    orc = O.from_volume(dt3._fm.keys, vol, (b, b))
    want = O.search(orc, tmpls, scene, 4, 4, kind=O.BATCH_OPTIMIZE, batch=4, nthreads=1)
    assert len(got) == len(want) > 0 and np.array_equal(got["tmpl_idx"], want["tmpl_idx"])
    assert np.allclose(got["score"], want["score"], rtol=1e-4, atol=1e-6)
    assert np.allclose(got["transform"], want["transform"], rtol=1e-4, atol=1e-6)
    again = fd.records_of(fd.search(fd.DefaultMatch(), fd.DefaultSearch(4, 4), fd.BatchOptimize(4), fd.Dt3Cpu(None, _device=adopted),
                                    tmpls, scene))
    assert got.tobytes() == again.tobytes()
    # the pool hands the handle to the next frame
    del dt3, fmap
    nxt = fd.build_image_featuremap(image(48, 40), fd.Dt3CpuParameters(depth=6, dt3Coeff=5.0, distance=fd.L2), threshold=60)
    assert same_bits(nxt._fm.volume(), ref_volume(48, 40, 6, 0, O.L2, 3)[1])
    fd.clear_featuremap_pool()


def test_end_to_end_a_rectangle_is_found_where_it_is():
    import openfdcm_amd as fd
    from test_definitions_scoring import definition_map
    W, H, x0, y0, w, h = 160, 120, 57, 38, 46, 31
    img = np.full((H, W), 40, dtype=np.uint8)
    img[y0:y0 + h + 1, x0:x0 + w + 1] = 210                       # filled, corners at (x0, y0) and (x0 + w, y0 + h)
    tmpl = np.array([[0, 0, w, 0], [w, 0, w, h], [w, h, 0, h], [0, h, 0, 0]], dtype=np.float32).T
    depth = 6
    keys, vol = edge_ref.reference_volume(edge_ref.edge_labels(img, depth, 60), 0, depth, 5.0, O.L2)
    grid = (0, 0, W - w, H - h, 1, 1)
    dmap = definition_map(vol, tmpl, (0.0, 0.0), grid)
    assert np.isfinite(dmap).all()
    jy, ix = np.unravel_index(np.argmin(dmap), dmap.shape)       # the first minimum in grid order, as (score, grid index) ranks
    assert abs(ix - x0) <= 2 and abs(jy - y0) <= 2, (ix, jy)
    dt3 = fd.build_image_featuremap(img, fd.Dt3CpuParameters(depth=depth, dt3Coeff=5.0, distance=fd.L2), threshold=60)
    rec = fd.records_of(fd.exhaustive_peaks(dt3, [tmpl], radius=4, k=3, window=grid))
    assert len(rec) >= 1
    assert (rec[0]["transform"][2], rec[0]["transform"][5]) == (ix, jy)
    assert rec[0]["score"] == dmap[jy, ix] or np.isclose(rec[0]["score"], dmap[jy, ix], rtol=1e-5)
    del dt3
    fd.clear_featuremap_pool()
