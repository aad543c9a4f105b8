"""CPU-only checks of the detections suppressed by footprint overlap (include/fdcm.h, "Detections suppressed by footprint
overlap"): the numpy referee (nms_ref.py) equals its point-by-point form, and the library's host-only footprints equal the
referee's, int for int.  A process without a device has no template handle, so the footprints are taken through
fdcm_lines_footprints, the entry for packed lines; fdcm_templates_footprints runs the same function on the handle's copy
of the lines and is compared with it on the device (test_gpu_detect_nms.py)."""
import os

import numpy as np
import pytest

from nms_ref import EMPTY, LIM, box_of_lines, brute_nms, footprints, nms_ref
from peaks_ref import peaks
from test_gpu_detect import CS7, _centers
from test_gpu_exhaustive import SIZES, _templates_with_sizes


@pytest.fixture(scope="module")
def fd():
    import __graft_entry__ as g
    from openfdcm_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        g.build()
    import openfdcm_amd
    return openfdcm_amd


def ragged_templates():
    """The 24 ragged templates of test_gpu_detect.py: its generator and seed, on the width its feature map has (the
    oracle's build of the same scene; the device's volume equals it bit for bit)."""
    from openfdcm_amd import synthetic
    from oracle import oracle as O
    orc = O.build(synthetic.scene(256, 48, 9), depth=12, coeff=5.0, padding=1.2, distance=O.L2, nthreads=8, stop_after=1)
    return _templates_with_sizes(np.random.default_rng(23), orc.W / 1.2, SIZES)


# ---------------------------------------------------------------- the referee against its point-by-point form
def _random_case(rng, ny, nx, n_pairs, levels, nan_frac):
    """Best-map planes with ties and points without candidates, and pairs whose boxes differ in size and position."""
    scores = (rng.integers(0, levels, size=(ny, nx)).astype(np.float32) * np.float32(0.75))
    scores[rng.random(scores.shape) < nan_frac] = np.nan
    pairs = rng.integers(0, n_pairs, size=(ny, nx)).astype(np.int32)
    pairs[np.isnan(scores)] = -1
    boxes = np.zeros((n_pairs, 4), dtype=np.int32)
    for u in range(n_pairs):
        x, y = rng.integers(-6, 4, size=2)
        w, h = rng.integers(1, [3, 7, 12][u % 3] + 1, size=2)
        boxes[u] = [x, y, x + w - 1, y + h - 1]
    return scores, pairs, boxes


@pytest.mark.parametrize("seed", range(8))
def test_reference_equals_brute_force(seed):
    rng = np.random.default_rng(900 + seed)
    ny, nx = [(9, 12), (1, 1), (1, 12), (9, 1), (5, 7), (9, 12), (3, 4), (8, 11)][seed]
    scores, pairs, boxes = _random_case(rng, ny, nx, n_pairs=int(rng.integers(1, 7)), levels=[2, 3, 1, 50, 4, 1000, 2, 6][seed],
                                        nan_frac=[0, 0, 0.2, 0.1, 0.5, 0.05, 0.9, 0.3][seed])
    grid = (-3, 5, nx, ny, [1, 2, 3, 1][seed % 4], [1, 1, 2, 4][seed % 4])
    for permille in (0, 1, 250, 999, 1000):
        for k in (1, 3, 64):
            g, s, F = nms_ref(scores, pairs, boxes, grid, k, permille)
            want = brute_nms(scores, pairs, boxes, grid, k, permille)
            assert np.array_equal(g, want)
            assert np.array_equal(s.view(np.uint32), scores.reshape(-1)[want].view(np.uint32))
            tx, ty = grid[0] + (want % nx) * grid[4], grid[1] + (want // nx) * grid[5]
            b = boxes[pairs.reshape(-1)[want]]
            assert F.dtype == np.int32 and np.array_equal(F, b + np.stack([tx, ty, tx, ty], axis=1))
            if permille == 1000:  # nothing is suppressed: the first k points by key
                pg, ps = peaks(scores, k, 0, 0)
                assert np.array_equal(g, pg) and np.array_equal(s.view(np.uint32), ps.view(np.uint32))
            if permille == 0:  # no two footprints share a pixel
                for a in range(len(F)):
                    for c in range(a):
                        assert (min(F[a, 2], F[c, 2]) < max(F[a, 0], F[c, 0]) or min(F[a, 3], F[c, 3]) < max(F[a, 1], F[c, 1]))


def test_reference_suppression_by_hand():
    """Two pairs, a 2 x 2 and a 6 x 1 box, on a 1 x 6 row of equal scores: at 0 the wide box of point 1 removes every point
    whose box touches columns 1 .. 6; thresholds between the ratios keep exactly the expected points."""
    scores = np.zeros((1, 6), dtype=np.float32)
    pairs = np.int32([[0, 1, 0, 0, 0, 0]])
    boxes = np.int32([[0, 0, 1, 1], [0, 0, 5, 0]])
    grid = (0, 0, 6, 1, 1, 1)
    # point 0: [0,1]x[0,1]; it meets point 1's [1,6]x[0,0] in 1 pixel of a union of 9, and point 2's [2,3]x[0,1] nowhere
    assert nms_ref(scores, pairs, boxes, grid, 64, 0)[0].tolist() == [0, 2, 4]
    assert nms_ref(scores, pairs, boxes, grid, 64, 111)[0].tolist() == [0, 2, 4]  # 1000 > 111 * 9: point 1 still goes ..
    assert nms_ref(scores, pairs, boxes, grid, 64, 112)[0].tolist() == [0, 1]     # .. stays from 112 on, and takes the rest
    assert nms_ref(scores, pairs, boxes, grid, 2, 1000)[0].tolist() == [0, 1]
    assert nms_ref(np.full((2, 2), np.nan, dtype=np.float32), np.full((2, 2), -1), boxes, (0, 0, 2, 2, 1, 1), 5, 300)[0].size == 0


# ---------------------------------------------------------------- the library's footprints against the referee's
def _same_boxes(fd, tmpls, cs=None, pivots=None):
    from openfdcm_amd.engine import lines_footprints
    for margin in (5, 0):
        got = lines_footprints(tmpls, cs, pivots, margin=margin)
        want = footprints(tmpls, cs, pivots, margin=margin)
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
    return want  # (margin 0)


def test_footprints_of_the_ragged_set(fd):
    tmpls = ragged_templates()
    piv = _centers(tmpls)
    none = _same_boxes(fd, tmpls)
    assert none.shape == (24, 1, 4) and none[0, 0].tolist() == list(EMPTY)
    assert len({(b[2] - b[0], b[3] - b[1]) for b in none[1:, 0]}) >= 20  # boxes of many sizes
    turned = _same_boxes(fd, tmpls, CS7, piv)
    assert turned.shape == (24, 7, 4) and np.all(turned[0] == EMPTY)
    assert not np.array_equal(turned[:, 0], turned[:, 3])
    scaled = CS7.copy()
    scaled[2] = [2, 0]  # an entry with scale
    big = _same_boxes(fd, tmpls, scaled, piv)
    assert np.all(big[1:, 2, 2] - big[1:, 2, 0] >= 2 * (none[1:, 0, 2] - none[1:, 0, 0]) - 2)
    assert np.array_equal(_same_boxes(fd, tmpls, CS7, None)[:, 0], none[:, 0])  # (1, 0) about the origin moves nothing
    # the public function: pivot "center", angles in radians
    pub = fd.template_footprints(tmpls, angles=np.deg2rad([0, 90]), margin=5)
    assert pub.shape == (24, 2, 4) and pub.dtype == np.int32
    cs = np.stack([np.cos(np.deg2rad([0, 90])), np.sin(np.deg2rad([0, 90]))], axis=1).astype(np.float32)
    assert np.array_equal(pub, footprints(tmpls, cs, piv, margin=5))
    assert np.array_equal(fd.template_footprints(tmpls), none)


def test_footprints_floor_signed_zero_and_clamp(fd):
    """floor, not truncation, of a negative fractional coordinate; -0.0 is 0; an empty template and a NaN end point give the
    empty box; huge and infinite coordinates clamp to +-2^25."""
    L = lambda *rows: np.array(rows, dtype=np.float32).T.copy()
    tmpls = [L((-0.5, -3.25, 2.75, 7.0)), np.zeros((4, 0), dtype=np.float32), L((-0.0, 0.0, -0.0, -0.0)),
             L((1, 2, 3, 4), (5, np.nan, 7, 8)), L((-1e30, 3e9, 4e7, np.inf)), L((-7.0, -7.000001, 6.9999995, 7.0)),
             L((33554430.0, -33554430.0, 33554432.0, -33554432.0))]
    want = _same_boxes(fd, tmpls)[:, 0]
    assert want[0].tolist() == [-1, -4, 2, 7]
    assert want[1].tolist() == list(EMPTY) and want[3].tolist() == list(EMPTY)
    assert want[2].tolist() == [0, 0, 0, 0]
    assert want[4].tolist() == [-LIM, LIM, LIM, LIM]
    assert want[5].tolist() == [-7, -8, 6, 7]
    assert want[6].tolist() == [LIM - 2, -LIM, LIM, -LIM + 2]
    from openfdcm_amd.engine import lines_footprints
    assert lines_footprints(tmpls, margin=5)[0, 0].tolist() == [-6, -9, 7, 12]
    assert lines_footprints(tmpls, margin=5)[6, 0].tolist() == [LIM - 7, -LIM, LIM, -LIM + 7]
    assert lines_footprints(tmpls, margin=4096)[1, 0].tolist() == list(EMPTY)
    with np.errstate(invalid="ignore", over="ignore"):  # 0 * inf in the referee's rotation: NaN there and in the library
        _same_boxes(fd, tmpls, np.float32([[0, 1], [-1, 0], [0.5, 0.5]]), np.float32([[1, 1]] * len(tmpls)))
    assert lines_footprints([]).shape == (0, 1, 4)
    assert box_of_lines(tmpls[0]).tolist() == [-1, -4, 2, 7]
