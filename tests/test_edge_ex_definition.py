"""Known answers of tests/edge_ex_ref.py, the numpy statement of include/fdcm.h's "edges with smoothing, hysteresis and a
minimum chain length": counts that pin the referee, inputs on which hysteresis differs from either threshold alone, the
serpentine whose far end is thousands of neighbour steps from its strong pixels, and the identity with the single-threshold
rule.  No library, no GPU."""
import numpy as np
import pytest

import edge_ex_ref as X
import edge_ref

# (width, height, seed, smooth, low, high, min_pixels) -> (candidates, strong, edge pixels)
COUNTS = [
    ((48, 40, 1, 0, 20, 60, 1), (616, 200, 395)),
    ((48, 40, 1, 0, 20, 60, 8), (616, 200, 385)),
    ((48, 40, 1, 1, 20, 60, 1), (315, 164, 164)),
    ((97, 61, 2, 1, 20, 60, 1), (868, 183, 211)),
    ((97, 61, 2, 0, 30, 100, 1), (1571, 186, 192)),
    ((130, 200, 130200, 0, 20, 60, 1), (8842, 1127, 5330)),
    ((130, 200, 130200, 0, 20, 60, 8), (8842, 1127, 5093)),
]


@pytest.mark.parametrize("case,want", COUNTS, ids=lambda v: "-".join(map(str, v)))
def test_known_counts_and_hysteresis_differs_from_both_thresholds(case, want):
    w, h, seed, smooth, low, high, min_pixels = case
    img = edge_ref.synthetic_image(w, h, seed)
    edge, cand, strong, _, _ = X.edge_mask(img, smooth, low, high, min_pixels)
    assert (int(cand.sum()), int(strong.sum()), int(edge.sum())) == want
    assert not (edge & ~cand).any() and not (strong & ~cand).any()
    S = X.smooth_image(img, smooth)
    at_low, at_high = edge_ref.edge_mask(S, low)[0], edge_ref.edge_mask(S, high)[0]
    assert np.array_equal(at_low, cand) and np.array_equal(at_high, strong)
    if want[2] not in (want[0], want[1]):
        assert not np.array_equal(edge, at_low) and not np.array_equal(edge, at_high)
    if min_pixels == 1:
        assert not (strong & ~edge).any()          # every strong pixel is kept, and what is kept touches a kept pixel or is strong
        comp, n = X.components(cand)
        assert set(np.unique(comp[edge])) == set(np.unique(comp[strong]))


def test_min_pixels_only_removes_whole_small_components():
    img = edge_ref.synthetic_image(48, 40, 1)
    e1, cand, _, _, _ = X.edge_mask(img, 0, 20, 60, 1)
    e8 = X.edge_mask(img, 0, 20, 60, 8)[0]
    comp, n = X.components(cand)
    size = np.bincount(comp[cand], minlength=n)
    gone = e1 & ~e8
    assert not (e8 & ~e1).any() and gone.sum() == 10
    assert (size[comp[gone]] < 8).all() and (size[comp[e8]] >= 8).all()


def test_smoothing_by_hand():
    img = np.zeros((3, 4), dtype=np.uint8)
    img[1, 1] = 255
    s1 = X.smooth_image(img, 1)
    assert s1[1, 1] == (4 * 255 + 8) >> 4 and s1[0, 0] == (255 + 8) >> 4 and s1[1, 3] == 0 and s1[0, 1] == (2 * 255 + 8) >> 4
    s2 = X.smooth_image(img, 2)
    assert s2[1, 1] == (36 * 255 + 128) >> 8 and s2[1, 3] == (6 * 255 + 128) >> 8
    corner = np.zeros((3, 4), dtype=np.uint8)
    corner[0, 0] = 255                               # the replicated border: I(-1, -1), I(-1, 0), I(0, -1) are the corner too
    assert X.smooth_image(corner, 1)[0, 0] == (9 * 255 + 8) >> 4
    assert X.smooth_image(corner, 2)[0, 0] == (121 * 255 + 128) >> 8
    flat = np.full((5, 7), 255, dtype=np.uint8)
    assert (X.smooth_image(flat, 1) == 255).all() and (X.smooth_image(flat, 2) == 255).all()
    assert np.array_equal(X.smooth_image(img, 0), img)


def test_serpentine_is_one_component_far_from_its_strong_pixels():
    img = X.serpentine(130, 200)
    assert img.shape == (200, 130)
    edge, cand, strong, _, _ = X.edge_mask(img, 0, 20, 100, 1)
    comp, n = X.components(cand)
    assert n == 1 and cand.sum() == 5900 and strong.sum() == 37
    assert np.array_equal(edge, cand)
    steps, reached = X.farthest_steps(cand, strong)
    assert reached == 5900 and steps == 2920 and steps > 2000


def test_serpentine_without_the_ramp_has_no_edge():
    img = X.serpentine(130, 200, ramp=False)
    edge, cand, strong, _, _ = X.edge_mask(img, 0, 20, 100, 1)
    assert cand.sum() == 5900 and strong.sum() == 0 and edge.sum() == 0
    assert (X.edge_labels(img, 30, 0, 20, 100, 1) == 255).all()


def test_wide_serpentine():
    img = X.serpentine(200, 130)
    assert img.shape == (130, 200)
    edge, cand, strong, _, _ = X.edge_mask(img, 0, 20, 100, 1)
    assert X.components(cand)[1] == 1 and cand.sum() == 5786 and np.array_equal(edge, cand)
    assert X.farthest_steps(cand, strong)[0] > 2000


@pytest.mark.parametrize("t", [1, 60, 1442])
def test_one_threshold_is_the_existing_rule(t):
    for (w, h, seed) in [(48, 40, 1), (97, 61, 2)]:
        img = edge_ref.synthetic_image(w, h, seed)
        for depth in (6, 30):
            assert np.array_equal(X.edge_labels(img, depth, 0, t, t, 1), edge_ref.edge_labels(img, depth, t))
    step = np.zeros((12, 70), dtype=np.uint8)
    step[5:, 33:] = 255
    assert np.array_equal(X.edge_labels(step, 30, 0, t, t, 1), edge_ref.edge_labels(step, 30, t))


def test_parameters_are_checked():
    img = np.zeros((4, 4), dtype=np.uint8)
    for bad in [(3, 20, 60, 1), (-1, 20, 60, 1), (0, 0, 60, 1), (0, 61, 60, 1), (0, 20, 1443, 1), (0, 20, 60, 0)]:
        with pytest.raises(ValueError):
            X.edge_mask(img, *bad)
