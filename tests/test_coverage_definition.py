"""Known answers of the referee of scene coverage (tests/coverage_ref.py; include/fdcm.h, "Scene coverage"), worked by hand, and
the section's identities on the referee.  No device.

The label image is 16 x 12 with m = 6 slices (depth 6: the keys -90, -60, .., 60 degrees).  A horizontal line has bin 3, a
vertical one bin 0.  The counts below are lattice points of a stadium: for a horizontal segment of L pixels and radius 3 the row
of the segment holds L + 6, the rows at distance 1 and 2 hold L + 4 (dx^2 <= 8, dx^2 <= 5: dx <= 2), the rows at distance 3 hold L."""
import numpy as np
import pytest

import coverage_ref as CR
from edge_ref import keys_of

W, H, M = 16, 12, 6
KEYS = keys_of(6)
HOR = np.float32([[4], [5], [11], [5]])     # 8 pixels, bin 3
VER = np.float32([[7], [3], [7], [8]])      # 6 pixels, bin 0
DIA = np.float32([[4], [3], [9], [8]])      # 6 pixels on the 45 degree diagonal
DOT = np.float32([[8], [6], [8], [6]])      # zero length
ALL = np.full((H, W), 3, dtype=np.uint8)    # every pixel an edge


def cover(labels, templates, poses, border=0, **kw):
    h, w = labels.shape
    return CR.coverage(labels, KEYS, (border, border), w + 2 * border, h + 2 * border, templates, poses, **kw)


def test_keys_and_bins():
    assert len(KEYS) == M
    assert CR.line_bins(HOR, KEYS)[0] == 3 and CR.line_bins(VER, KEYS)[0] == 0
    assert CR.line_bins(np.float32([[0], [0], [6], [3]]), KEYS)[0] == 4      # 26.6 degrees: nearest 30
    assert CR.line_bins(np.float32([[0], [0], [1], [-2]]), KEYS)[0] == 1     # -63.4 degrees: nearest -60


# (template, radius) -> (edges = the window's area at margin = radius, explained), tolerance m / 2 on the all-edge image
KNOWN = [(HOR, 0, 8, 8), (HOR, 1, 30, 26), (HOR, 3, 98, 78),
         (VER, 0, 6, 6), (VER, 1, 24, 20), (VER, 3, 84, 64),
         (DIA, 0, 36, 6), (DIA, 1, 64, 20), (DIA, 3, 144, 74),
         (DOT, 0, 1, 1), (DOT, 1, 9, 5), (DOT, 3, 49, 29)]


@pytest.mark.parametrize("tm,radius,edges,explained", KNOWN)
def test_segments_on_the_all_edge_image(tm, radius, edges, explained):
    counts, residual, masks = cover(ALL, [tm], [[0, 0, 0, 0]], radius=radius, bin_tolerance=3)
    assert tuple(counts[0]) == (edges, explained)
    assert (residual == 255).sum() == explained and np.array_equal(residual == 255, masks[0])
    # the same set from the distance to the segment in float64 (the radii are far from any tie but exact ones: 1e-9 settles them)
    a, b = np.float64(tm[:2, 0]), np.float64(tm[2:, 0])
    d = b - a
    for py in range(H):
        for px in range(W):
            p = np.float64([px, py])
            t = 0.0 if not d.any() else min(1.0, max(0.0, float((p - a) @ d) / float(d @ d)))
            near = float(np.sum((p - (a + t * d)) ** 2)) <= radius * radius + 1e-9
            assert masks[0][py, px] == near, (px, py)


def test_the_three_branches_point_by_point():
    seg = (4, 5, 11, 5)
    assert CR.near_segment(2, 5, *seg, 2) and not CR.near_segment(2, 5, *seg, 1)        # beyond A: the first end cap
    assert CR.near_segment(13, 5, *seg, 2) and not CR.near_segment(13, 5, *seg, 1)      # beyond B: the second end cap
    assert CR.near_segment(7, 7, *seg, 2) and not CR.near_segment(7, 7, *seg, 1)        # the interior: the cross product
    assert CR.near_segment(3, 6, *seg, 2) and not CR.near_segment(3, 6, *seg, 1)        # dot < 0, distance^2 = 2
    dia = (4, 3, 9, 8)
    assert CR.near_segment(3, 2, *dia, 2) and not CR.near_segment(3, 2, *dia, 1)        # beyond A on the diagonal: distance^2 = 2
    assert CR.near_segment(10, 9, *dia, 2) and not CR.near_segment(10, 9, *dia, 1)
    assert CR.near_segment(5, 3, *dia, 1) and not CR.near_segment(6, 3, *dia, 1)        # cross^2 = 25, 100 against 50
    assert CR.near_segment(8, 6, 8, 6, 8, 6, 0) and not CR.near_segment(8, 7, 8, 6, 8, 6, 0)   # A = B
    big = 1 << 40                                                                        # Python integers: exact at any size
    assert CR.near_segment(big // 2, 1, 0, 0, big, 0, 1) and not CR.near_segment(big // 2, 2, 0, 0, big, 0, 1)


def test_python_integers_and_int64_arrays_agree():
    rng = np.random.default_rng(5)
    ys, xs = np.mgrid[0:40, 0:40]
    for _ in range(60):
        ax, ay, bx, by = (int(v) for v in rng.integers(-5, 45, size=4))
        r = int(rng.integers(0, 33))
        got = CR.near_segment_many(xs.ravel(), ys.ravel(), ax, ay, bx, by, r)
        want = [CR.near_segment(x, y, ax, ay, bx, by, r) for x, y in zip(xs.ravel(), ys.ravel())]
        assert np.array_equal(got, want)


@pytest.mark.parametrize("label,want", [(0, (6, 6, 6)), (5, (0, 6, 6)), (1, (0, 6, 6)), (2, (0, 0, 6)), (4, (0, 0, 6)), (3, (0, 0, 6)),
                                        (6, None), (254, None), (255, None)])
def test_bin_tolerance_0_1_and_half(label, want):
    """A vertical template (bin 0) on its own pixels labelled `label`: |0 - 5| wraps to 1; 6 .. 255 are no edge."""
    labels = np.full((H, W), 255, dtype=np.uint8)
    labels[3:9, 7] = label
    for tol, n in zip((0, 1, 3), want or (0, 0, 0)):
        counts, residual, _ = cover(labels, [VER], [[0, 0, 0, 0]], radius=0, bin_tolerance=tol, margin=2)
        assert tuple(counts[0]) == ((6, n) if want else (0, 0))
        assert (residual != labels).sum() == n and np.all(residual[residual != labels] == 255)


def test_window_clipping_at_the_four_borders_and_empty_windows():
    kw = dict(radius=1, bin_tolerance=3)
    counts, _, _ = cover(ALL, [HOR], [[0, 0, -4, 0], [0, 0, 4, 0], [0, 0, 0, -5], [0, 0, 0, 6], [0, 0, -5, 0], [0, 0, 5, 0]], **kw)
    assert [tuple(c) for c in counts] == [(27, 25), (27, 25), (20, 18), (20, 18), (-1, -1), (-1, -1)]
    # a map with a border holds poses whose window misses the image
    counts, residual, masks = cover(ALL, [HOR, np.zeros((4, 0), np.float32)], [[0, 0, 0, -9], [0, 0, -9, 0], [0, 0, -10, 0], [1, 0, 3, 3]],
                                    border=5, **kw)
    assert [tuple(c) for c in counts] == [(0, 0), (12, 10), (-1, -1), (0, 0)]   # x = -9: columns -5 .. 2 -> window 0 .. 3
    assert masks[2] is None and not masks[0].any() and not masks[3].any()
    assert (residual == 255).sum() == 10
    # margin alone widens the window, never the explained set
    a, _, _ = cover(ALL, [HOR], [[0, 0, 0, 0]], radius=1, bin_tolerance=3, margin=0)
    b, _, _ = cover(ALL, [HOR], [[0, 0, 0, 0]], radius=1, bin_tolerance=3, margin=40)
    assert tuple(a[0]) == (8, 8) and tuple(b[0]) == (W * H, 26)


def _random_case(seed):
    rng = np.random.default_rng(seed)
    labels = np.where(rng.uniform(size=(H, W)) < 0.3, rng.integers(0, M, size=(H, W)), 255).astype(np.uint8)
    tmpls = [rng.integers(2, 10, size=(4, n)).astype(np.float32) for n in (1, 3, 5)]
    poses = np.stack([rng.integers(0, 3, 12), np.zeros(12, int), rng.integers(-6, 9, 12), rng.integers(-6, 6, 12)], axis=1)
    return rng, labels, tmpls, poses


@pytest.mark.parametrize("seed", range(6))
def test_identities(seed):
    rng, labels, tmpls, poses = _random_case(seed)
    base = None
    for radius in (0, 1, 2, 5):
        prev = None
        for tol in (0, 1, 2, 3):
            counts, residual, masks = cover(labels, tmpls, poses, radius=radius, bin_tolerance=tol, margin=3)
            adm = counts[:, 0] >= 0
            assert np.all(counts[adm, 1] <= counts[adm, 0]) and np.all(counts[~adm] == -1)
            if prev is not None:
                assert np.all(counts[:, 1] >= prev[:, 1]) and np.array_equal(counts[:, 0], prev[:, 0])
            prev = counts
        if base is not None:
            assert np.all(prev[:, 1] >= base[:, 1]) and np.array_equal(prev[:, 0], base[:, 0])   # radius grows at a fixed margin
        base = prev
    # bin_tolerance = m / 2: only "is an edge" matters
    other = np.where(labels < M, rng.integers(0, M, size=labels.shape), labels).astype(np.uint8)
    a, ra, _ = cover(labels, tmpls, poses, radius=2, bin_tolerance=3)
    b, rb, _ = cover(other, tmpls, poses, radius=2, bin_tolerance=3)
    assert np.array_equal(a, b) and np.array_equal(ra == 255, rb == 255)
    # the residual of a concatenation is the "255 if either" of the parts; duplicates change nothing
    c1, r1, _ = cover(labels, tmpls, poses[:5], radius=2, bin_tolerance=1)
    c2, r2, _ = cover(labels, tmpls, poses[5:], radius=2, bin_tolerance=1)
    c, r, _ = cover(labels, tmpls, poses, radius=2, bin_tolerance=1)
    assert np.array_equal(c, np.concatenate([c1, c2])) and np.array_equal(r, np.where((r1 == 255) | (r2 == 255), 255, labels))
    cd, rd, _ = cover(labels, tmpls, np.concatenate([poses, poses]), radius=2, bin_tolerance=1)
    assert np.array_equal(cd, np.concatenate([c, c])) and np.array_equal(rd, r)
    # no edges: (0, 0) and the labels themselves
    none = np.full((H, W), 255, dtype=np.uint8)
    none[2, 3], none[5, 5] = M, 254
    c0, r0, _ = cover(none, tmpls, poses, radius=2, bin_tolerance=1)
    assert np.all(c0[c[:, 0] >= 0] == 0) and np.array_equal(c0 < 0, c < 0) and np.array_equal(r0, none)
    # n = 0
    ce, re_, _ = cover(labels, tmpls, np.zeros((0, 4), int))
    assert ce.shape == (0, 2) and np.array_equal(re_, labels)
