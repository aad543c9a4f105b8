"""Known answers for tests/edge_ref.py, the numpy statement of the image definitions (include/fdcm.h, "feature maps from
images").  CPU only: the oracle's closest_orientation bins the angles with the host libm."""
import numpy as np
import pytest

import edge_ref
from oracle import oracle as O


def vertical_step(W=12, H=9, at=6, lo=20, hi=200):
    img = np.full((H, W), lo, dtype=np.uint8)
    img[:, at:] = hi
    return img


def test_sobel_of_a_ramp_and_the_replicate_border():
    img = (np.arange(7, dtype=np.uint8) * 10)[None, :].repeat(5, axis=0)
    gx, gy, m2 = edge_ref.sobel(img)
    assert (gy == 0).all()
    assert (gx[:, 1:-1] == 80).all() and (gx[:, 0] == 40).all() and (gx[:, -1] == 40).all()   # 4 * 2 * 10; half at the clamped ends
    assert (m2 == gx * gx).all()


def test_vertical_step_gives_one_column_with_the_vertical_key():
    img = vertical_step()
    depth = 6
    lab = edge_ref.edge_labels(img, depth, 60)
    cols = np.flatnonzero((lab != edge_ref.NO_EDGE).any(axis=0))
    assert list(cols) == [5]                                  # the -d side of the plateau (columns 5 and 6 have the same m2)
    assert (lab[:, 5] != edge_ref.NO_EDGE).all()
    keys = edge_ref.keys_of(depth)
    # gx > 0, gy = 0: tangent (+0, gx), angle +pi/2, which wraps to the key at -pi/2 (slice 0), the vertical one
    assert (lab[:, 5] == 0).all() and keys[0] == np.float32(-np.pi / 2)
    assert O.closest_orientation(keys, (0.0, 0.0, 0.0, 5.0)) == 0


def test_two_pixel_plateau_keeps_the_pixel_on_the_minus_d_side():
    img = vertical_step()
    gx, gy, m2 = edge_ref.sobel(img)
    assert m2[4, 5] == m2[4, 6] > 0 and m2[4, 4] == 0 and m2[4, 7] == 0
    edge, _, _ = edge_ref.edge_mask(img, 1)
    assert edge[:, 5].all() and not edge[:, 6].any()
    # a horizontal step, d = (0, 1): the upper row of the two wins
    edge, _, _ = edge_ref.edge_mask(np.ascontiguousarray(img.T), 1)
    assert edge[5, :].all() and not edge[6, :].any()


def test_axis_gradients_fall_into_the_end_and_middle_bins():
    depth = 6
    keys = edge_ref.keys_of(depth)
    v = edge_ref.edge_labels(vertical_step(), depth, 60)                              # gy = 0, gx > 0: dx = +0, angle +pi/2
    assert set(np.unique(v)) == {0, edge_ref.NO_EDGE}
    v = edge_ref.edge_labels(vertical_step(lo=200, hi=20), depth, 60)                 # gy = 0, gx < 0: angle -pi/2
    assert set(np.unique(v)) == {0, edge_ref.NO_EDGE}
    h = edge_ref.edge_labels(np.ascontiguousarray(vertical_step().T), depth, 60)     # gx = 0: dy = +0, angle -0 -> key 0.0
    mid = int(np.argmin(np.abs(keys)))
    assert keys[mid] == 0 and set(np.unique(h)) == {mid, edge_ref.NO_EDGE}
    h = edge_ref.edge_labels(np.ascontiguousarray(vertical_step(lo=200, hi=20).T), depth, 60)
    assert set(np.unique(h)) == {mid, edge_ref.NO_EDGE}


def test_diagonal_direction_follows_the_signs():
    n = 16
    yy, xx = np.mgrid[0:n, 0:n]
    down = np.where(xx + yy >= n, 200, 20).astype(np.uint8)    # gx > 0, gy > 0: d = (1, 1)
    up = np.where(xx - yy >= 0, 200, 20).astype(np.uint8)      # gx > 0, gy < 0: d = (1, -1)
    for img, sy in ((down, 1), (up, -1)):
        edge, gx, gy = edge_ref.edge_mask(img, 60)
        _, _, m2 = edge_ref.sobel(img)
        ys, xs = np.nonzero(edge[3:-3, 3:-3])
        assert len(ys) >= 10
        for y, x in zip(ys + 3, xs + 3):                     # along d = (1, sy): strictly above the pixel before, not below the one after
            assert m2[y, x] > m2[y - sy, x - 1] and m2[y, x] >= m2[y + sy, x + 1]
            assert not (edge[y - sy, x - 1] and m2[y - sy, x - 1] == m2[y, x])
    lab = edge_ref.edge_labels(down, 4, 60)
    keys = edge_ref.keys_of(4)
    assert set(np.unique(lab[3:-3, 3:-3])) == {int(np.argmin(np.abs(keys + np.float32(np.pi / 4)))), edge_ref.NO_EDGE}


def test_constant_image_has_no_edge():
    for v in (0, 77, 255):
        lab = edge_ref.edge_labels(np.full((9, 13), v, dtype=np.uint8), 30, 1)
        assert (lab == edge_ref.NO_EDGE).all()


@pytest.mark.parametrize("thr", [0, -3, 1443, 100000])
def test_threshold_bounds_are_enforced(thr):
    with pytest.raises(ValueError):
        edge_ref.edge_labels(vertical_step(), 6, thr)


def test_threshold_extremes():
    img = np.zeros((8, 8), dtype=np.uint8)
    img[:, 4:] = 255                                           # |gx| = 1020, the largest a straight step gives
    assert (edge_ref.edge_labels(img, 6, 1020) != edge_ref.NO_EDGE).any()
    assert (edge_ref.edge_labels(img, 6, 1021) == edge_ref.NO_EDGE).all()
    corner = np.zeros((8, 8), dtype=np.uint8)
    corner[4:, 4:] = 255
    _, _, m2 = edge_ref.sobel(corner)
    assert m2.max() <= 2 * 1020 ** 2 < 1443 ** 2               # why 1442 is the last threshold that can select anything


def test_reference_volume_stage1_zeros_are_the_labelled_pixels():
    img = edge_ref.synthetic_image(48, 40, 1)
    lab = edge_ref.edge_labels(img, 6, 60)
    for border in (0, 3):
        keys, vol = edge_ref.reference_volume(lab, border, 6, 5.0, O.L2_SQUARED, stop_after=1)
        assert vol.shape == (6, 48 + 2 * border, 40 + 2 * border)
        for k in range(6):
            ys, xs = np.nonzero(lab == k)
            z = np.zeros(vol[k].shape, dtype=bool)
            z[xs + border, ys + border] = True
            assert np.array_equal(vol[k] == 0, z)
    blank = np.full((5, 7), 255, dtype=np.uint8)
    _, vol = edge_ref.reference_volume(blank, 0, 2, 5.0, O.L2_SQUARED, stop_after=1)
    assert (vol == edge_ref.FMAX).all()
    _, vol = edge_ref.reference_volume(blank, 0, 2, 5.0, O.L2, stop_after=1)
    assert (vol == np.sqrt(edge_ref.FMAX)).all()


def test_synthetic_images_use_every_bin():
    small = edge_ref.edge_labels(edge_ref.synthetic_image(48, 40, 1), 6, 60)
    assert set(np.unique(small)) == set(range(6)) | {edge_ref.NO_EDGE}
    big = edge_ref.edge_labels(edge_ref.synthetic_image(97, 61, 2), 30, 60)
    assert set(np.unique(big)) == set(range(30)) | {edge_ref.NO_EDGE}
    assert (small != edge_ref.NO_EDGE).sum() >= 100 and (big != edge_ref.NO_EDGE).sum() >= 200
