"""The image pyramid on the GPU (include/fdcm.h, "image pyramid") against tests/pyramid_ref.py: level images over the sizes that
matter to the 64 x 16 tile, from host and device memory; the feature map of a level against the feature map of the referee's level
image; rebuilds on one handle and the pool; lifted records read by pose_windows and found again by a level-0 search; the drivers
against their written-out composition; and the end-to-end case of tests/pyramid_scene.py.  Every comparison is on bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

import edge_ref
import pyramid_ref as R
import pyramid_scene as S

pytestmark = pytest.mark.gpu

# 1 x 1, thinner than the kernel's reach, an exact fit of the tile and of two tiles, one pixel under and over, odd sizes whose
# last source column or row is read by the clamp only, more than one block each way
SIZES = [(1, 1), (2, 1), (3, 5), (63, 15), (64, 16), (65, 17), (127, 33), (129, 31), (130, 35), (257, 130)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def content(width, height, kind):
    if kind == "random":
        img = np.random.default_rng(width * 1000 + height).integers(0, 256, size=(height, width), dtype=np.uint8)
    elif kind == "white":
        img = np.full((height, width), 255, dtype=np.uint8)
    else:
        yy, xx = np.mgrid[0:height, 0:width]
        img = (((xx + yy) & 1) * 255).astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def want_level(width, height, kind, level):
    img = content(width, height, kind) if level == 0 else R.down(want_level(width, height, kind, level - 1))
    img.setflags(write=False)
    return img


def collapse_level(width, height):
    level = 0
    while R.level_size(width, height, level) != (1, 1):
        level += 1
    return max(level, 1)


def levels_of(width, height):
    return sorted({1, 2, 3, 4, collapse_level(width, height)})


# ---------------------------------------------------------------- 1. level images
@pytest.mark.parametrize("width,height", SIZES, ids=lambda v: str(v))
def test_level_images_equal_the_referee_from_host_memory(width, height):
    import openfdcm_amd as fd
    assert collapse_level(width, height) <= R.MAX_LEVEL
    for kind in ("random", "white", "checker"):
        img = content(width, height, kind)
        assert np.array_equal(fd.image_pyramid(img, 0), img)
        for level in levels_of(width, height):
            want = want_level(width, height, kind, level)
            got = fd.image_pyramid(img, level)
            assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == want.shape, (kind, level)
            assert np.array_equal(got, want), (kind, level, np.argwhere(got != want)[:5])
            if kind == "white":
                assert (got == 255).all()
    wide = np.full((height, width + 3), 0xA5, dtype=np.uint8)       # row_stride > width
    wide[:, :width] = content(width, height, "random")
    view = wide[:, :width]
    assert view.strides[0] == width + 3 or height == 1
    for level in [0] + levels_of(width, height):
        assert np.array_equal(fd.image_pyramid(view, level), want_level(width, height, "random", level)), level
    assert want_level(width, height, "random", collapse_level(width, height)).shape == (1, 1)


@pytest.mark.parametrize("width,height", SIZES, ids=lambda v: str(v))
def test_level_images_equal_the_referee_from_device_memory(width, height):
    import torch

    import openfdcm_amd as fd
    from openfdcm_amd import _capi
    img = content(width, height, "random")
    n = width * height
    levels = levels_of(width, height)
    t = torch.from_numpy(np.array(img)).cuda()
    for level in [0] + levels:
        got = fd.image_pyramid(t, level)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), want_level(width, height, "random", level)), level
    wide = torch.full((height, width + 3), 0xA5, dtype=torch.uint8, device="cuda")   # rows 3 bytes longer, read in place
    wide[:, :width] = t
    for level in levels:
        assert np.array_equal(fd.image_pyramid(wide[:, :width], level).cpu().numpy(), want_level(width, height, "random", level)), level
    for off in (1, 2, 3):                                            # a device pointer misaligned by 1, 2 and 3 bytes
        flat = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        flat[off:off + n] = t.reshape(-1)
        view = flat[off:off + n].view(height, width)
        assert view.data_ptr() % 4 == off
        for level in levels:
            assert np.array_equal(fd.image_pyramid(view, level).cpu().numpy(), want_level(width, height, "random", level)), (off, level)
    # out_on_device = 1 into the middle of a buffer: the bytes around the output stay
    for level in [0] + levels:
        want = want_level(width, height, "random", level)
        before, after = 37, 29
        out = torch.full((before + want.size + after,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _capi.check(_capi.lib().fdcm_image_pyramid_level(C.c_void_p(t.data_ptr()), width, height, width, 1, level,
                                                         C.c_void_p(out.data_ptr() + before), 1))
        host = out.cpu().numpy()
        assert (host[:before] == 0xA5).all() and (host[before + want.size:] == 0xA5).all(), level
        assert np.array_equal(host[before:before + want.size].reshape(want.shape), want), level
    # host in, device out and device in, host out
    want = want_level(width, height, "random", levels[0])
    out = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _capi.check(_capi.lib().fdcm_image_pyramid_level(C.c_void_p(img.ctypes.data), width, height, width, 0, levels[0],
                                                     C.c_void_p(out.data_ptr()), 1))
    assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)
    back = np.zeros(want.shape, dtype=np.uint8)
    _capi.check(_capi.lib().fdcm_image_pyramid_level(C.c_void_p(t.data_ptr()), width, height, width, 1, levels[0],
                                                     C.c_void_p(back.ctypes.data), 0))
    assert np.array_equal(back, want)


# ---------------------------------------------------------------- 2. - 5. feature maps of a level
@functools.lru_cache(maxsize=None)
def picture(width, height):
    img = edge_ref.synthetic_image(width, height, width * 1000 + height)
    img.setflags(write=False)
    return img


EDGE_OPTIONS = [dict(), dict(low=20), dict(smooth=2), dict(low=25, smooth=1, min_pixels=6)]


def _same_map(a, b):
    assert (a.width, a.height, a.depth) == (b.width, b.height, b.depth)
    assert np.array_equal(a.scene_translation, b.scene_translation) and np.array_equal(a.keys, b.keys)
    assert same_bits(a.volume(), b.volume())


@pytest.mark.parametrize("opts", EDGE_OPTIONS, ids=lambda v: str(v))
def test_level_0_is_build_image(opts):
    from openfdcm_amd.engine import DeviceFeatureMap
    img = picture(130, 75)
    for border in (0, 3):
        a = DeviceFeatureMap.build_image_level(img, 0, 60, border=border, depth=12, **opts)
        b = DeviceFeatureMap.build_image(img, 60, border=border, depth=12, **opts)
        assert (a.width, a.height) == (130 + 2 * border, 75 + 2 * border) and a.scene_translation.tolist() == [border, border]
        _same_map(a, b)
        assert np.isfinite(a.volume()).any()
        a.close(); b.close()


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("opts", EDGE_OPTIONS, ids=lambda v: str(v))
def test_level_map_is_build_image_of_the_referees_level_image(level, opts):
    import torch

    from openfdcm_amd.engine import DeviceFeatureMap
    img = picture(261, 131)                                          # odd sizes: W_1 = 131, H_1 = 66, W_2 = 66, H_2 = 33
    small = R.level_image(img, level)
    for border in (0, 3):
        a = DeviceFeatureMap.build_image_level(img, level, 50, border=border, depth=30, **opts)
        b = DeviceFeatureMap.build_image(small, 50, border=border, depth=30, **opts)
        assert (a.width, a.height) == (small.shape[1] + 2 * border, small.shape[0] + 2 * border)
        assert a.scene_translation.tolist() == [border, border]
        _same_map(a, b)
        vol = a.volume()
        assert np.isfinite(vol).all() and len(np.unique(vol)) > 100      # (edges were found at this level)
        a.close()
        if border == 3:                                              # the same from device memory with long rows, and L1
            wide = torch.full((131, 264), 0xA5, dtype=torch.uint8, device="cuda")
            wide[:, :261] = torch.from_numpy(np.array(img)).cuda()
            c = DeviceFeatureMap.build_image_level(wide[:, :261], level, 50, border=border, depth=30, **opts)
            _same_map(c, b)
            c.close()
        b.close()


def test_one_handle_through_levels_sizes_and_seed_kinds():
    from openfdcm_amd import _capi
    from openfdcm_amd.engine import DeviceFeatureMap
    img, little = picture(261, 131), picture(97, 61)
    opts = dict(low=25, smooth=1, min_pixels=4)
    scene = np.array([[10, 12, 60, 40], [70, 20, 30, 90], [5, 100, 120, 110]], dtype=np.float32).T
    fm = DeviceFeatureMap.build_image_level(img, 2, 50, border=1, depth=30, **opts)
    fresh = DeviceFeatureMap.build_image_level(img, 2, 50, border=1, depth=30, **opts)
    _same_map(fm, fresh); fresh.close()
    # a refused rebuild leaves the handle as it was
    p = C.c_void_p(img.ctypes.data)
    e = _capi.EdgeParams(1, 25, 50, 4)
    before = fm.volume()
    for args, what in [((261, 131, 261, 0, 13, C.byref(e), 1), "level"), ((261, 131, 261, 0, -1, C.byref(e), 1), "level"),
                       ((261, 131, 261, 0, 1, None, 1), "params is null"), ((261, 131, 260, 0, 1, C.byref(e), 1), "row_stride"),
                       ((4097, 131, 4097, 0, 1, C.byref(e), 1), "4096"), ((261, 131, 261, 0, 1, C.byref(e), -1), "border")]:
        assert _capi.lib().fdcm_featuremap_rebuild_image_level(fm._h, p, *args) == -1
        assert what in _capi.lib().fdcm_last_error().decode()
    assert _capi.lib().fdcm_featuremap_rebuild_image_level(fm._h, None, 261, 131, 261, 0, 1, C.byref(e), 1) == -1
    fm.refresh()
    assert (fm.width, fm.height) == (68, 35) and same_bits(fm.volume(), before)

    fm.rebuild_image_level(img, 0, 50, border=2, **opts)
    fresh = DeviceFeatureMap.build_image(img, 50, border=2, depth=30, **opts)
    _same_map(fm, fresh); fresh.close()
    fm.rebuild(scene)
    fresh = DeviceFeatureMap.build(scene, depth=30, coeff=5.0, padding=0.0)
    _same_map(fm, fresh); fresh.close()
    fm.rebuild_image_level(img, 1, 50, border=0, **opts)
    fresh = DeviceFeatureMap.build_image(R.level_image(img, 1), 50, border=0, depth=30, **opts)
    _same_map(fm, fresh); fresh.close()
    fm.rebuild_image_level(little, 3, 40, border=2)
    fresh = DeviceFeatureMap.build_image(R.level_image(little, 3), 40, border=2, depth=30)
    assert (fm.width, fm.height) == (13 + 4, 8 + 4)
    _same_map(fm, fresh); fresh.close()
    fm.close()


def test_the_pool_keeps_levels_apart():
    import openfdcm_amd as fd
    from openfdcm_amd.engine import DeviceFeatureMap
    fd.clear_featuremap_pool()
    img, other = picture(261, 131), picture(130, 75)
    params = fd.Dt3CpuParameters(depth=30, dt3Coeff=5.0)
    a = fd.build_image_featuremap_level(img, 1, params, threshold=50, border=1, smooth=1)
    handle = a._fm
    want = DeviceFeatureMap.build_image(R.level_image(img, 1), 50, border=1, depth=30, smooth=1)
    _same_map(a._fm, want); want.close()
    del a                                                            # its handle goes to the pool under its level
    c = fd.build_image_featuremap_level(other, 2, params, threshold=50)
    assert c._fm is not handle
    want = DeviceFeatureMap.build_image(R.level_image(other, 2), 50, depth=30)
    _same_map(c._fm, want); want.close()
    b = fd.build_image_featuremap_level(other, 1, params, threshold=50, low=20)
    assert b._fm is handle                                           # the same level: the pooled handle, rebuilt
    want = DeviceFeatureMap.build_image(R.level_image(other, 1), 50, depth=30, low=20)
    _same_map(b._fm, want); want.close()
    plain = fd.build_image_featuremap(other, params, threshold=50)
    assert plain._fm is not handle and plain._fm is not c._fm
    del b, c, plain
    fd.clear_featuremap_pool()


# ---------------------------------------------------------------- 6. lifted records
def _small_templates(rng, n=4):
    """Templates of a few lines inside a box of 30 x 24 pixels, integer and half-integer end points."""
    return [np.ascontiguousarray((rng.integers(0, 60, size=(4, int(k))) * np.array([[0.5], [0.4], [0.5], [0.4]])).astype(np.float32))
            for k in rng.integers(2, 6, size=n)]


@pytest.mark.parametrize("pivot", ["center", None])
def test_lifted_records_name_the_level_0_pose(pivot):
    import openfdcm_amd as fd
    rng = np.random.default_rng(5)
    img = np.array(edge_ref.synthetic_image(96, 80, 11))
    tmpls = _small_templates(rng)
    small = fd.scaled_templates(tmpls, 1)
    params = fd.Dt3CpuParameters(depth=12, dt3Coeff=5.0)
    fm1 = fd.build_image_featuremap_level(img, 1, params, threshold=50, border=2)
    # (border 6 at level 0: every pose admissible on the level-1 map, -1 < p/2 + 2 + t < 52, is admissible there at 2 t)
    fm0 = fd.build_image_featuremap(img, params, threshold=50, border=6)
    assert fm1.get_feature_size().tolist() == [52, 44] and fm0.get_feature_size().tolist() == [108, 92]
    angles = np.deg2rad(np.arange(0, 360, 45.0) + 3.0)
    cs = fd._angles(angles)
    pv = fd.template_pivots(tmpls, pivot)
    pv1 = None if pv is None else pv * np.float32(0.5)
    recs = fd.exhaustive_rotation_search(fm1, small, angles, k=16, pivot=pv1).records()
    plain = fd.exhaustive_search(fm1, small, k=8).records()            # pure translations: the table of the one angle 0
    assert len(recs) == 16 * len(tmpls) and len(plain) == 8 * len(tmpls)
    for rec, table, piv, piv1, search_angles in [(recs, angles, pv, pv1, angles), (plain, np.zeros(1), None, None, None)]:
        tab = fd._angles(table)
        want = np.zeros((len(rec), 7), dtype=np.int32)
        for q, r in enumerate(rec):                                    # the level's pose by the documented rule, not by pose_windows
            tr, t = r["transform"], int(r["tmpl_idx"])
            a = int(np.nonzero((tab[:, 0] == tr[0]) & (tab[:, 1] == tr[3]))[0][0])
            p1 = np.zeros(2, dtype=np.float32) if piv1 is None else piv1[t]
            m = R.record_transform(tab[a, 0], tab[a, 1], p1, (0, 0))
            tl = (int(np.rint(float(tr[2]) - float(m[2]))), int(np.rint(float(tr[5]) - float(m[5]))))
            rule = R.record_transform(tab[a, 0], tab[a, 1], p1, tl)     # (a pure translation writes +0 where the rule has -s = -0)
            assert np.array_equal(rule, tr) and np.array_equal(rule[[0, 2, 3, 5]].view(np.uint32), tr[[0, 2, 3, 5]].view(np.uint32))
            want[q] = (t, a, 1, 2 * tl[0], 2 * tl[1], 1, 1)
        up = fd.lift_records(rec, 1)
        jobs = fd.pose_windows(up, table, table, piv, 0, 0, 0)
        assert np.array_equal(jobs, want)
        assert len({tuple(j) for j in jobs}) > len(jobs) // 2
        # ... and a level-0 search at exactly that pose emits the lifted record, bit for bit
        back, off = fd.exhaustive_window_search(fm0, tmpls, jobs, angles=search_angles, pivot=piv)
        assert off.tolist() == list(range(len(jobs) + 1))
        assert back.records()["transform"].tobytes() == up["transform"].tobytes()
        assert np.array_equal(back.records()["tmpl_idx"], up["tmpl_idx"])


# ---------------------------------------------------------------- 7. the drivers are their compositions
@pytest.fixture(scope="module")
def maps():
    """The scene's maps at depth 30 (the drivers' identities need no fine orientation table): level 0, 1 and 2."""
    import openfdcm_amd as fd
    params = fd.Dt3CpuParameters(depth=30, dt3Coeff=S.COEFF)
    img = S.frame()
    kw = dict(threshold=S.EDGE["threshold"], low=S.EDGE["low"], smooth=S.EDGE["smooth"], min_pixels=S.EDGE["min_pixels"])
    out = {0: fd.build_image_featuremap(img, params, border=4, **kw)}
    for level in (1, 2):
        out[level] = fd.build_image_featuremap_level(img, level, params, border=2, **kw)
    return out


def _parts(res):
    res = res if isinstance(res, tuple) else (res,)
    return [np.ascontiguousarray(p.records() if hasattr(p, "records") else p).tobytes() for p in res]


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("case", ["center", "explicit", "origin+wrap", "hull+gate", "one angle"])
def test_drivers_equal_their_written_out_composition(maps, level, case):
    import openfdcm_amd as fd
    tmpls = S.templates() + [np.array([[0, 0, 25, 0], [25, 0, 25, 18]], dtype=np.float32).T]
    coarse, fine = np.deg2rad(np.arange(0, 360, 20.0)), np.deg2rad(np.arange(0, 360, 4.0))
    pivot, wrap, gate, mm = "center", False, "winner", None
    if case == "explicit":
        pivot = np.array([[3, -2], [0.5, 7], [12.5, 9]], dtype=np.float32)
    elif case == "origin+wrap":
        pivot, wrap = None, True
    elif case == "hull+gate":
        tmpls, gate, mm = fd.with_footprint(tmpls, "hull"), "all", 0.4
    elif case == "one angle":
        coarse = fine = np.zeros(1)
    pen = fd.DefaultPenalty()
    f = np.float32(2.0 ** -level)
    common = dict(penalty=pen, pivot=pivot, wrap=wrap, margin=3, line_caps=4.0, min_matched=mm, gate=gate, overlap=0.3, max_detections=20)
    out = dict(return_boxes=True, return_matched=True, return_jobs=True)

    small = fd.scaled_templates(tmpls, level)
    pv = fd.template_pivots(tmpls, pivot)
    seeds_l = fd.exhaustive_detect_all(maps[level], small, float("inf"), overlap=0.5, stride=1, max_detections=24, penalty=pen, angles=coarse,
                                       pivot=None if pv is None else pv * f, line_caps=2.0, margin=-(-3 >> level))
    assert 12 <= len(seeds_l) <= 24
    jobs = fd.pose_windows(fd.lift_records(seeds_l, level), coarse, fine, pv, 2, 2 ** level, 2 ** level, stride=1, wrap=wrap)
    want = fd.exhaustive_detect_windows(maps[0], tmpls, jobs, 6.0, angles=fine, stride=1, **common, **out)
    got = fd.exhaustive_detect_pyramid(maps[0], maps[level], level, tmpls, 6.0, coarse, fine, 2, coarse_overlap=0.5, coarse_max_detections=24,
                                       coarse_line_caps=2.0, **common, **out)
    assert len(got) == 4 and isinstance(got[0], fd.MatchList) and len(got[0]) >= 2
    assert _parts(got) == _parts(want)
    assert np.array_equal(got[3], want[3]) and got[3].max() < 24      # the job indices are the seeds'
    alone = fd.exhaustive_detect_pyramid(maps[0], maps[level], level, tmpls, 6.0, coarse, fine, 2, coarse_overlap=0.5, coarse_max_detections=24,
                                         coarse_line_caps=2.0, **common)
    assert isinstance(alone, fd.MatchList) and _parts(alone) == _parts(want)[:1]
    # explicit half widths, margin and coarse threshold
    thr = float(np.sort(seeds_l.records()["score"])[len(seeds_l) // 2])
    few = fd.exhaustive_detect_all(maps[level], small, thr, overlap=0.5, stride=1, max_detections=24, penalty=pen, angles=coarse,
                                   pivot=None if pv is None else pv * f, line_caps=2.0, margin=1)
    assert 1 <= len(few) < len(seeds_l)
    jobs2 = fd.pose_windows(fd.lift_records(few, level), coarse, fine, pv, 2, 1, 3, stride=1, wrap=wrap)
    want2 = fd.exhaustive_detect_windows(maps[0], tmpls, jobs2, 6.0, angles=fine, stride=1, **common, **out)
    got2 = fd.exhaustive_detect_pyramid(maps[0], maps[level], level, tmpls, 6.0, coarse, fine, 2, half_x=1, half_y=3, coarse_max_score=thr,
                                        coarse_overlap=0.5, coarse_max_detections=24, coarse_line_caps=2.0, coarse_margin=1, **common, **out)
    assert _parts(got2) == _parts(want2)

    objects = np.array([0, 1, 0], dtype=np.int32)
    ocommon = dict(common, cross_overlap=0.6, n_objects=2)
    oout = dict(out, return_objects=True)
    seeds_o = fd.exhaustive_detect_objects(maps[level], small, objects, float("inf"), overlap=0.5, cross_overlap=0.9, stride=1,
                                           max_detections=24, penalty=pen, angles=coarse, pivot=None if pv is None else pv * f,
                                           line_caps=2.0, margin=-(-3 >> level), n_objects=2)
    jobs_o = fd.pose_windows(fd.lift_records(seeds_o, level), coarse, fine, pv, 2, 2 ** level, 2 ** level, stride=1, wrap=wrap)
    want_o = fd.exhaustive_detect_windows_objects(maps[0], tmpls, jobs_o, objects, [6.0, 5.0], angles=fine, stride=1, **ocommon, **oout)
    got_o = fd.exhaustive_detect_pyramid_objects(maps[0], maps[level], level, tmpls, objects, [6.0, 5.0], coarse, fine, 2, coarse_overlap=0.5,
                                                 coarse_cross_overlap=0.9, coarse_max_detections=24, coarse_line_caps=2.0, **ocommon, **oout)
    assert len(got_o) == 5 and len(got_o[0]) >= 2 and _parts(got_o) == _parts(want_o)


# ---------------------------------------------------------------- 8. end to end
@pytest.fixture(scope="module")
def scene_maps():
    import openfdcm_amd as fd
    params = fd.Dt3CpuParameters(depth=S.DEPTH, dt3Coeff=S.COEFF)
    img = S.frame()
    kw = dict(border=S.BORDER, threshold=S.EDGE["threshold"], low=S.EDGE["low"], smooth=S.EDGE["smooth"], min_pixels=S.EDGE["min_pixels"])
    out = {0: fd.build_image_featuremap(img, params, **kw)}
    for level in (1, 2):
        out[level] = fd.build_image_featuremap_level(img, level, params, **kw)
    return out


@pytest.mark.parametrize("level", [1, 2])
def test_end_to_end_the_planted_parts_are_found(scene_maps, level):
    """Three filled polygons of two shapes: the pyramid chain at this level returns three detections, each its planted template
    within 1 px and one fine angle step, and so does the strided chain with coarse_stride = 2^level."""
    import openfdcm_amd as fd
    tmpls = S.templates()
    kw = dict(coarse_overlap=S.COARSE_OVERLAP, coarse_max_detections=S.COARSE_MAX, penalty=fd.DefaultPenalty(), pivot=None, wrap=True,
              overlap=0.3)
    dets = fd.exhaustive_detect_pyramid(scene_maps[0], scene_maps[level], level, tmpls, S.MAX_SCORE, S.COARSE, S.FINE, S.HALF_ANGLES, **kw)
    rec = dets.records()
    print("pyramid level", level, [(int(r["tmpl_idx"]), float(r["score"]), r["transform"][[2, 5]].tolist()) for r in rec])
    assert S.recovered(rec) == ([True, True, True], 3)
    half = 2 ** level
    dets = fd.exhaustive_detect_refined(scene_maps[0], tmpls, S.MAX_SCORE, S.COARSE, S.FINE, half, S.HALF_ANGLES, half, half, **kw)
    rec = dets.records()
    print("refined stride", half, [(int(r["tmpl_idx"]), float(r["score"]), r["transform"][[2, 5]].tolist()) for r in rec])
    assert S.recovered(rec) == ([True, True, True], 3)
