"""Line segments from label images on the GPU (include/fdcm.h, "line segments from images") against tests/lines_ref.py: the
synthetic images over the sizes that matter to the 64 x 16 tile, hand-made label images that pin one rule each, random labels,
the image and device entry points, repeated calls, the blank image, and one frame taken end to end.  Every comparison with the
referee is on the float32 bits and on the order."""
import functools

import numpy as np
import pytest

import edge_ex_ref as X
import edge_ref
import lines_ref as L
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (4, 1), (5, 3), (64, 16), (65, 17), (48, 40), (97, 61), (61, 97), (130, 200), (700, 9), (12, 2100)]
EDGES = [(1, 20, 60, 1), (0, 60, 60, 1)]          # (smooth, low, high, min_pixels): hysteresis on a smoothed image; threshold 60
DEPTHS = (6, 30, 180)
LINE_PARAMS = [(2, 1), (8, 8)]                    # (min_pixels, min_length)
NONE = np.uint8(255)


def same_lines(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return (got.dtype == want.dtype == np.float32 and got.shape == want.shape and got.shape[0] == 4
            and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)))


@functools.lru_cache(maxsize=None)
def image(width, height, seed=None):
    img = edge_ref.synthetic_image(width, height, width * 1000 + height if seed is None else seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def labels_of_image(width, height, depth, edge):
    lab = X.edge_labels(image(width, height), depth, *edge)
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def referee_of_image(width, height, depth, edge, bucket, min_pixels, min_length):
    m = len(edge_ref.keys_of(depth))
    return L.segments(labels_of_image(width, height, depth, edge), m, bucket, min_pixels, min_length)


def buckets_of(depth):
    m = len(edge_ref.keys_of(depth))
    return sorted({1, min(4, m), min(6, m), m})


def check(lab, depth, bucket, min_pixels, min_length):
    """The library's segments of `lab`, equal to the referee's; returns (segments, the referee's info)."""
    import openfdcm_amd
    want, info = L.segments(lab, len(edge_ref.keys_of(depth)), bucket, min_pixels, min_length)
    got = openfdcm_amd.lines_from_labels(lab, depth=depth, bucket=bucket, line_pixels=min_pixels, line_length=min_length)
    assert same_lines(got, want), (got.shape, want.shape, got.T[:4], want.T[:4])
    return got, info


# ---------------------------------------------------------------- 1. synthetic images
@pytest.mark.parametrize("width,height", SIZES, ids=lambda v: str(v))
def test_segments_of_synthetic_images_equal_the_definition(width, height):
    import openfdcm_amd
    for edge in EDGES:
        for depth in DEPTHS:
            lab = labels_of_image(width, height, depth, edge)
            for bucket in buckets_of(depth):
                for min_pixels, min_length in LINE_PARAMS:
                    want, _ = referee_of_image(width, height, depth, edge, bucket, min_pixels, min_length)
                    got = openfdcm_amd.lines_from_labels(lab, depth=depth, bucket=bucket, line_pixels=min_pixels, line_length=min_length)
                    assert same_lines(got, want), (edge, depth, bucket, min_pixels, min_length, got.shape, want.shape)


def test_the_synthetic_set_has_kept_b_components_and_exact_halves():
    """From the referee alone: the set above exercises partition B's output and the strict majority's tie."""
    kept_b = ties = segments = 0
    for width, height in [(97, 61), (61, 97), (130, 200)]:
        for bucket in (4, 6):
            seg, info = referee_of_image(width, height, 30, EDGES[0], bucket, 8, 8)
            kept_b += info["kept_b"]; ties += info["ties"]; segments += seg.shape[1]
    assert kept_b > 0 and ties > 0 and segments > kept_b


# ---------------------------------------------------------------- 2. hand-made label images
def blank(width, height):
    return np.full((height, width), NONE, dtype=np.uint8)


def test_one_row_across_eleven_tiles_and_its_transpose():
    lab = blank(700, 9)
    lab[4, :] = 7
    got, info = check(lab, 30, 4, 8, 8)
    assert info["keys"] == [2 * 4 * 700] and np.array_equal(got.T, np.float32([[0, 4, 699, 4]]))
    got, info = check(np.ascontiguousarray(lab.T), 30, 4, 8, 8)
    assert info["keys"] == [2 * 4] and np.array_equal(got.T, np.float32([[4, 0, 4, 699]]))


def test_labels_on_a_bucket_boundary_are_whole_in_partition_b():
    w = 4
    lab = blank(90, 70)
    for i in range(60):
        lab[5 + i, 9 + i] = w - 1 + (i & 1)
    got, info = check(lab, 30, w, 8, 8)
    assert info["keys"] == [2 * (5 * 90 + 9) + 1] and np.array_equal(got.T, np.float32([[9, 5, 68, 64]]))
    assert check(lab, 30, 1, 2, 1)[0].shape == (4, 0)          # bucket 1: sixty components of one pixel


def test_the_labels_wrap():
    lab = blank(150, 20)
    lab[11, 3:140] = np.where(np.arange(137) & 1, 0, 29)
    got, info = check(lab, 30, 4, 8, 8)
    assert info["keys"] == [2 * (11 * 150 + 3) + 1] and np.array_equal(got.T, np.float32([[3, 11, 139, 11]]))
    got, info = check(lab, 30, 30, 8, 8)                        # one bucket: A holds everything, and wins the tie
    assert info["keys"] == [2 * (11 * 150 + 3)]


def test_a_serpentine_of_one_label():
    lab = X.edge_labels(X.serpentine(130, 200), 30, 0, 20, 100, 1)
    lab = np.where(lab != 255, np.uint8(5), NONE).astype(np.uint8)
    assert int((lab != 255).sum()) == 5900
    got, info = check(lab, 30, 4, 8, 8)
    assert len(info["pixels"][0][0]) > 2000                      # the band is one component (two contours at most)
    check(np.ascontiguousarray(lab.T), 30, 4, 8, 8)


def test_the_largest_component_kept_and_the_smallest_dropped():
    lab = blank(300, 280)
    lab[5:5 + 257, 3:3 + 255] = 11                               # 65535 pixels
    got, info = check(lab, 30, 4, 8, 8)
    assert got.shape == (4, 1) and len(info["pixels"][0][0]) == 65535
    lab[5:5 + 257, 3:3 + 256] = 11                               # 65792
    assert check(lab, 30, 4, 8, 8)[0].shape == (4, 0)


def test_two_pixels_at_each_corner():
    lab = blank(70, 20)
    lab[0, 0:2] = 3; lab[0:2, 69] = 3; lab[19, 68:70] = 3; lab[18:20, 0] = 3
    got, info = check(lab, 30, 4, 2, 1)
    assert got.shape == (4, 4) and info["keys"] == [0, 2 * 69, 2 * (18 * 70), 2 * (19 * 70 + 68)]
    assert check(lab, 30, 4, 2, 3)[0].shape == (4, 0)


def test_touching_components_of_different_buckets_stay_apart():
    lab = blank(80, 30)
    lab[10, 5:70] = 1
    lab[11, 5:70] = 9
    got, info = check(lab, 30, 4, 8, 8)
    assert np.array_equal(got.T, np.float32([[5, 10, 69, 10], [5, 11, 69, 11]]))
    lab[11, 5:70] = 2                                            # the same bucket in A: one component of two rows
    got, info = check(lab, 30, 4, 8, 8)
    assert got.shape == (4, 1) and len(info["pixels"][0][0]) == 130


# ---------------------------------------------------------------- 3. fuzz
@pytest.mark.parametrize("width,height", [(97, 61), (65, 17)], ids=lambda v: str(v))
def test_random_labels(width, height):
    ties = kept = 0
    for seed in range(20):
        rng = np.random.default_rng(1000 * width + seed)
        lab = np.where(rng.random((height, width)) < 0.5, rng.integers(0, 30, (height, width)), 255).astype(np.uint8)
        got, info = check(lab, 30, 4, 2, 1)
        ties += info["ties"]; kept += got.shape[1]
    assert kept > 20 * 10 and ties > 0


def test_random_labels_past_one_pass_of_either_scan():
    """601 x 587: more than 256 blocks of 1024 pixels and more than 256 blocks of 256 components, so the scan of the root counts
    and the scan of the kept counts both carry a sum from one pass of their workgroup to the next."""
    width, height = 601, 587
    rng = np.random.default_rng(7)
    lab = np.where(rng.random((height, width)) < 0.5, rng.integers(0, 30, (height, width)), 255).astype(np.uint8)
    _, a, b = L.buckets(lab, 30, 4)
    assert width * height > 256 * 1024 and L.components(a)[1] + L.components(b)[1] > 256 * 256
    got, info = check(lab, 30, 4, 3, 2)
    assert got.shape[1] > 10000 and info["kept_b"] > 1000


# ---------------------------------------------------------------- 4. image and device entry points
OPTS = dict(depth=30, threshold=60, low=20, smooth=1, min_pixels=1)
LINE = dict(bucket=4, line_pixels=8, line_length=8)


def strided(img, extra=3):
    buf = np.full((img.shape[0], img.shape[1] + extra), 0xA5, dtype=np.uint8)
    buf[:, :img.shape[1]] = img
    return buf[:, :img.shape[1]]


def test_lines_from_image_are_those_of_its_labels():
    import torch

    import openfdcm_amd as fd
    for width, height in [(97, 61), (130, 200)]:
        img = image(width, height)
        for opts in (OPTS, dict(depth=30, threshold=60), dict(depth=6, threshold=100, low=30, smooth=2, min_pixels=3)):
            lab = fd.edge_labels(img, **opts)
            want, _ = L.segments(lab, len(edge_ref.keys_of(opts["depth"])), 4, 8, 8)
            assert want.shape[1] > 0
            assert same_lines(fd.lines_from_labels(lab, depth=opts["depth"], **LINE), want)
            assert same_lines(fd.lines_from_image(img, **opts, **LINE), want)
            assert same_lines(fd.lines_from_image(strided(img), **opts, **LINE), want)
            assert same_lines(fd.lines_from_labels(strided(lab), depth=opts["depth"], **LINE), want)
            t = torch.from_numpy(np.array(img)).cuda()
            wide = torch.full((height, width + 3), 0xA5, dtype=torch.uint8, device="cuda")
            wide[:, :width] = t
            assert same_lines(fd.lines_from_image(t, **opts, **LINE), want)
            assert same_lines(fd.lines_from_image(wide[:, :width], **opts, **LINE), want)
            assert same_lines(fd.lines_from_labels(torch.from_numpy(lab).cuda(), depth=opts["depth"], **LINE), want)
    with pytest.raises(ValueError, match="contiguous"):
        fd.lines_from_labels(wide[:, :width], depth=30)


# ---------------------------------------------------------------- 5. repeated calls
def test_repeated_and_alternated_calls_give_the_same():
    import openfdcm_amd as fd
    a, b = image(130, 200), image(48, 40)
    first = {id(img): fd.lines_from_image(img, **OPTS, **LINE) for img in (a, b)}
    assert first[id(a)].shape[1] > 0 and first[id(b)].shape[1] > 0
    for img in (a, a, b, a, b, b, a):
        assert same_lines(fd.lines_from_image(img, **OPTS, **LINE), first[id(img)])
    lab = labels_of_image(130, 200, 30, EDGES[0])
    one = fd.lines_from_labels(lab, **LINE)
    small = np.full((3, 5), 2, dtype=np.uint8)
    for _ in range(2):
        assert fd.lines_from_labels(small, bucket=4, line_pixels=2, line_length=1).shape == (4, 1)
        assert same_lines(fd.lines_from_labels(lab, **LINE), one)
    t = fd.engine.lines_last_timing()
    assert t["n_lines"] == one.shape[1] and t["edges_ms"] == 0 and t["total_ms"] > 0


# ---------------------------------------------------------------- 6. blank
def test_a_blank_label_image_gives_no_lines_and_no_error():
    import openfdcm_amd as fd
    for width, height in [(1, 1), (48, 40), (130, 200)]:
        got = fd.lines_from_labels(blank(width, height), depth=30)
        assert got.shape == (4, 0) and got.dtype == np.float32
    assert fd.lines_from_image(np.full((40, 48), 90, dtype=np.uint8), **OPTS).shape == (4, 0)
    # labels at and above m are no edges either
    assert fd.lines_from_labels(np.full((40, 48), 6, dtype=np.uint8), depth=6, bucket=1).shape == (4, 0)


# ---------------------------------------------------------------- 7. end to end
def quadrilateral():
    """(96, 96) uint8: a filled quadrilateral without a symmetry, 210 on 40."""
    pts = np.array([(10, 30), (60, 8), (88, 50), (40, 86)], dtype=np.float64)
    yy, xx = np.mgrid[0:96, 0:96]
    inside = np.ones((96, 96), dtype=bool)
    for i in range(4):
        (ax, ay), (bx, by) = pts[i], pts[(i + 1) % 4]
        inside &= (bx - ax) * (yy - ay) - (by - ay) * (xx - ax) >= 0
    img = np.full((96, 96), 40, dtype=np.uint8)
    img[inside] = 210
    return img


def test_end_to_end_a_picture_becomes_the_template_that_finds_it():
    import openfdcm_amd as fd
    ox, oy, depth = 71, 38, 30
    picture = quadrilateral()
    scene = np.full((192, 256), 40, dtype=np.uint8)
    scene[oy:oy + 96, ox:ox + 96] = picture
    edge = (1, 20, 60, 1)
    # on the CPU first: the referee's template on the oracle's volume of the scene's labels
    lab_s = X.edge_labels(scene, depth, *edge)
    tmpl_ref, _ = L.segments(X.edge_labels(picture, depth, *edge), 30, 4, 8, 8)
    assert tmpl_ref.shape == (4, 4)
    keys, vol = edge_ref.reference_volume(lab_s, 0, depth, 5.0, O.L2)
    orc = O.from_volume(keys, vol, (0, 0))
    xs, ys = tmpl_ref[[0, 2]].ravel(), tmpl_ref[[1, 3]].ravel()
    tx = np.arange(int(np.ceil(-xs.min())), int(np.floor(255 - xs.max())) + 1)
    ty = np.arange(int(np.ceil(-ys.min())), int(np.floor(191 - ys.max())) + 1)
    T = np.array([(x, y) for y in ty for x in tx], dtype=np.float32)
    best = T[np.nanargmin(O.evaluate(orc, tmpl_ref, T))]
    assert abs(best[0] - ox) <= 1 and abs(best[1] - oy) <= 1, best
    # the library: picture -> template, frame -> feature map, every translation scored
    opts = dict(depth=depth, threshold=60, low=20, smooth=1, min_pixels=1)
    tmpl = fd.lines_from_image(picture, **opts, **LINE)
    assert same_lines(tmpl, tmpl_ref)
    params = fd.Dt3CpuParameters(depth=depth, dt3Coeff=5.0, distance=fd.L2)
    dt3 = fd.build_image_featuremap(scene, params, threshold=60, low=20, smooth=1)
    rec = fd.records_of(fd.exhaustive_search(dt3, [tmpl], stride=1, k=1))
    assert len(rec) == 1
    found = (rec[0]["transform"][2], rec[0]["transform"][5])
    assert abs(found[0] - ox) <= 1 and abs(found[1] - oy) <= 1, found
    # search(), the reference's path, on the frame's own lines
    scene_lines = fd.lines_from_image(scene, **opts, **LINE)
    assert same_lines(scene_lines, L.segments(lab_s, 30, 4, 8, 8)[0]) and scene_lines.shape == (4, 4)
    assert np.allclose(scene_lines, tmpl + np.float32([[ox], [oy], [ox], [oy]]), rtol=0, atol=1e-3)
    got = fd.records_of(fd.search(fd.DefaultMatch(), fd.DefaultSearch(4, 4), fd.BatchOptimize(4), dt3, [tmpl], scene_lines))
    want = O.search(O.from_volume(dt3._fm.keys, dt3._fm.volume(), (0, 0)), [tmpl], scene_lines, 4, 4, kind=O.BATCH_OPTIMIZE, batch=4, nthreads=1)
    assert len(got) == len(want) > 0 and np.array_equal(got["tmpl_idx"], want["tmpl_idx"])
    assert np.allclose(got["score"], want["score"], rtol=1e-4, atol=1e-6)
    assert np.allclose(got["transform"], want["transform"], rtol=1e-4, atol=1e-6)
    del dt3
    fd.clear_featuremap_pool()
