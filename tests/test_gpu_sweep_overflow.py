"""The balanced L2 / L2^2 sweep where its on-chip stages run out: rows whose stacks and owner lists are far longer than
the LDS rings (8 entries per row and range) and the owner walk's LDS window (64 entries per row) hold, so that the
scratch behind them -- written and read back by the same workgroup -- carries the row.  Whole volumes, bit for bit
against the CPU oracle.

The scenes reach the scratch by what they are, not by a switch: every test first counts, from the oracle's own
distance transform, the owners of a row (runs of pixels with the same argmin column of f[u] + (x - u)^2) and asserts
that the count exceeds the window, so that a scene cannot silently stop covering the spill.
"""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

WALK_WINDOW = 64    # owner entries per row the owner walk keeps in LDS (kWin, fdcm_sweep.hip); older ones come back from scratch
FILL_ROUND = 10     # owner entries per row and round of the fill (kRE)
RING = 8            # stack entries per (row, range) in LDS (kRing)
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def amd():
    import openfdcm_amd
    from openfdcm_amd import _capi
    import ctypes as C
    n = C.c_int()
    _capi.check(_capi.lib().fdcm_device_count(C.byref(n)))
    assert n.value >= 1, "no HIP device visible"
    return openfdcm_amd


def lines(*segs):
    return np.array(segs, dtype=np.float32).T.reshape(4, -1)


def vertical_lines(W, H, step):
    """Parallel lines `step` pixels apart along x, each over the whole height: every `step`-th column is seeded in every row."""
    return lines(*[(x, 0, x, H - 1) for x in range(0, W, step)] + ([(W - 1, 0, W - 1, H - 1)] if (W - 1) % step else []))


def diagonals(W, H):
    return lines((0, 0, W - 1, H - 1), (0, H - 1, W - 1, 0))


def owners_per_row(dt_sq_slice, rows):
    """dt_sq_slice: one slice [x][y] of the oracle's L2^2 transform (exact integers).  Its zeros are the seeds; pass 1 is
    f[u][y] = squared distance along y to the nearest seed of column u; the owner of pixel x in row y is the column u that
    minimises f[u][y] + (x - u)^2, the smallest on a tie.  Returns the number of owner runs of each of `rows`."""
    W, H = dt_sq_slice.shape
    seeds = dt_sq_slice == 0
    cols = np.nonzero(seeds.any(axis=1))[0]
    assert len(cols) > 0
    ys = np.arange(H, dtype=np.int64)
    xs = np.arange(W, dtype=np.int64)
    out = []
    for y in rows:
        f = np.array([((y - ys[seeds[u]]) ** 2).min() for u in cols], dtype=np.int64)
        cost = f[None, :] + (xs[:, None] - cols[None, :]) ** 2   # [pixel][seeded column]
        # (the reference reads the owner's value back in place where an entry takes over behind its own column, imgproc.h:126-127:
        # its transform is the envelope's value or, there, less)
        assert np.all(dt_sq_slice[:, y].astype(np.int64) <= cost.min(axis=1)), "pass 1 as restated here is not the oracle's"
        own = cost.argmin(axis=1)
        out.append(1 + int(np.count_nonzero(own[1:] != own[:-1])))
    return out


def densest_slice(dt_sq):
    return int(np.argmax((dt_sq == 0).sum(axis=(1, 2))))


def assert_volume_equal(dev, orc, what):
    a, b = dev.volume(), orc.volume()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = a.view(np.uint32) == b.view(np.uint32)
    if not same.all():
        bad = np.argwhere(~same)
        k, x, y = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {a.size} voxels differ; first at slice {k} x {x} y {y}: "
                             f"hip {a[k, x, y]!r} oracle {b[k, x, y]!r}")


def build_both(scene, depth, dist, stage=3):
    from openfdcm_amd.engine import DeviceFeatureMap
    dev = DeviceFeatureMap.build(scene, depth=depth, coeff=5.0, padding=1.0, distance=dist, stop_after=stage)
    orc = O.build(scene, depth=depth, coeff=5.0, padding=1.0, distance=dist, nthreads=8, stop_after=stage)
    return dev, orc


SCENES_A = {"lines-1px": lambda: vertical_lines(1024, 1024, 1), "lines-2px": lambda: vertical_lines(1024, 1024, 2),
            "diagonals": lambda: diagonals(1024, 1024)}


@pytest.mark.parametrize("dist", [O.L2, O.L2_SQUARED], ids=["L2", "L2_SQUARED"])
@pytest.mark.parametrize("name", sorted(SCENES_A))
def test_longest_owner_lists(amd, name, dist):
    """(a) 1024 x 1024, depth 30: lines one and two pixels apart along x (every, every other column owns pixels in every
    row: 1024 and 512 owners per row, the longest lists there are) and the two diagonals (the owner changes every other
    pixel).  Every row's list is many times the walk's window and the fill's round; its stack many times the ring."""
    scene = SCENES_A[name]()
    dt = O.build(scene, depth=30, coeff=5.0, padding=1.0, distance=O.L2_SQUARED, nthreads=8, stop_after=1).volume()
    assert dt.shape == (30, 1024, 1024)
    counts = owners_per_row(dt[densest_slice(dt)], [0, 1, 63, 64, 511, 777, 1023])
    print(f"{name}: owners per row {counts}")
    assert min(counts) >= 400 > 4 * WALK_WINDOW > FILL_ROUND > RING, counts
    dev, orc = build_both(scene, 30, dist)
    assert (dev.width, dev.height) == (1024, 1024)
    assert_volume_equal(dev, orc, f"{name} dist {dist}")
    dev1, orc1 = build_both(scene, 30, dist, stage=1)   # the sweep's own output, before propagation and integral
    assert_volume_equal(dev1, orc1, f"{name} dist {dist} stage 1")


@pytest.mark.parametrize("dist", [O.L2, O.L2_SQUARED], ids=["L2", "L2_SQUARED"])
def test_seedless_slice_next_to_a_dense_one(amd, dist):
    """(b) all lines of one orientation: its slice has a seed in every column and row, every other slice has none
    (FLT_MAX throughout, written by the workgroups that find no seeded column) -- neighbours in the volume and in the
    scratch's chunk order."""
    scene = vertical_lines(1024, 1024, 1)
    dt = O.build(scene, depth=30, coeff=5.0, padding=1.0, distance=O.L2_SQUARED, nthreads=8, stop_after=1).volume()
    k = densest_slice(dt)
    assert np.all(dt[k] == 0)
    others = [j for j in range(30) if j != k]
    assert all(np.all(dt[j] == FLT_MAX) for j in others), "a slice beside the dense one has seeds"
    assert owners_per_row(dt[k], [0, 1023]) == [1024, 1024]
    dev, orc = build_both(scene, 30, dist, stage=1)
    assert_volume_equal(dev, orc, f"dense and seedless slices, dist {dist}, stage 1")
    dev, orc = build_both(scene, 30, dist)
    assert_volume_equal(dev, orc, f"dense and seedless slices, dist {dist}")


@pytest.mark.parametrize("dist", [O.L2, O.L2_SQUARED], ids=["L2", "L2_SQUARED"])
@pytest.mark.parametrize("bw,bh", [(64, 2048), (2048, 64)])
def test_thin_scenes(amd, bw, bh, dist):
    """(c) scenes whose bounding boxes are 64 x 2048 and 2048 x 64.  A map built from a scene is square (the side is the
    box's larger extent, dt3cpu.cpp:109-116, here as in the reference), so there is no 64 x 2048 feature map to build: both
    scenes give 2048 x 2048 (2 * 2048^2 < 2^24: the balanced sweep takes them) with every seed in a strip of 64 columns,
    or of 64 rows, through the middle.  Lines two pixels apart along x and the box's diagonals: in the first the strip's 33
    columns own all 2048 pixels of every row, in the second every row, inside the strip and far from it, has a thousand owners."""
    S = 2048
    assert 2 * S * S <= 1 << 24
    scene = np.concatenate([vertical_lines(bw, bh, 2), diagonals(bw, bh)], axis=1)
    dt = O.build(scene, depth=6, coeff=5.0, padding=1.0, distance=O.L2_SQUARED, nthreads=8, stop_after=1).volume()
    assert dt.shape == (6, S, S)
    counts = owners_per_row(dt[densest_slice(dt)], [0, S // 2, S - 1])
    print(f"box {bw} x {bh}: owners per row {counts}")
    assert counts[1] >= (bw // 4 if bw <= WALK_WINDOW else 4 * WALK_WINDOW) > FILL_ROUND > RING, counts
    for stage in (1, 3):
        dev, orc = build_both(scene, 6, dist, stage=stage)
        assert (dev.width, dev.height) == (S, S)
        assert_volume_equal(dev, orc, f"box {bw} x {bh} dist {dist} stage {stage}")
