"""The referee of the detector with objects (objects_ref.py; include/fdcm.h, "Objects") against itself, without a device: the
numpy statement of the greedy rule agrees with the one in Python integers on random small planes, the hand-built cases the
definition was written for come out as stated, one object is nms_ref, and relabelling the objects changes nothing."""
import numpy as np
import pytest

import nms_ref
from objects_ref import brute_objects_nms, objects_best, objects_nms, objects_winner
from gate_ref import gated_best


def _random_case(seed, G=3, T=5, A=2, nx=7, ny=5):
    """Planes of G objects on a small grid: scores from a few values (ties on (q, g) across objects happen), pairs of the
    object's own templates, boxes of assorted sizes."""
    rng = np.random.default_rng(seed)
    objects = np.array([t % G for t in range(T)])
    objects[-1] = 0
    boxes = np.zeros((T * A, 4), dtype=np.int32)
    for u in range(T * A):
        w, h = rng.integers(0, 5, size=2)
        x, y = rng.integers(-3, 2, size=2)
        boxes[u] = (x, y, x + w, y + h)
    scores = rng.choice(np.float32([0, 0.25, 0.5, 0.5, 1.5, np.inf, np.nan]), size=(G, ny, nx)).astype(np.float32)
    pairs = np.full((G, ny, nx), -1, dtype=np.int32)
    for o in range(G):
        mine = [t * A + a for t in range(T) if objects[t] == o for a in range(A)]
        pairs[o] = rng.choice(mine, size=(ny, nx))
    pairs[np.isnan(scores)] = -1
    return scores, pairs, boxes, (-4, 3, nx, ny, 2, 1), objects


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("permille,cross", [(300, 300), (300, 1000), (0, 0), (500, 100), (1000, 0)])
def test_the_two_statements_agree(seed, permille, cross):
    scores, pairs, boxes, grid, objects = _random_case(seed)
    for md in (4096, 3):
        a = objects_nms(scores, pairs, boxes, grid, objects, md, permille, cross)
        b = brute_objects_nms(scores, pairs, boxes, grid, md, permille, cross)
        assert np.array_equal(a, b) and (md != 4096 or len(a) >= 3)
    if permille == cross == 0:  # no two footprints share a pixel
        F = [nms_ref.point_boxes(pairs[o], boxes, grid)[g] for o, g in a]
        for i in range(len(F)):
            for j in range(i):
                assert min(F[i][2], F[j][2]) < max(F[i][0], F[j][0]) or min(F[i][3], F[j][3]) < max(F[i][1], F[j][1])


def test_two_objects_at_one_point():
    """Equal boxes at one translation: both survive at cross = 1000, only the better one at cross = 0; neither outcome
    depends on overlap_permille, which only acts within an object."""
    boxes = np.int32([[0, 0, 9, 9], [0, 0, 9, 9]])
    objects = np.array([0, 1])
    scores = np.full((2, 1, 3), np.nan, dtype=np.float32)
    pairs = np.full((2, 1, 3), -1, dtype=np.int32)
    scores[0, 0, 1], pairs[0, 0, 1] = 0.5, 0
    scores[1, 0, 1], pairs[1, 0, 1] = 0.25, 1
    grid = (0, 0, 3, 1, 1, 1)
    for permille in (0, 300, 1000):
        both = objects_nms(scores, pairs, boxes, grid, objects, 10, permille, 1000)
        assert both.tolist() == [[1, 1], [0, 1]]
        one = objects_nms(scores, pairs, boxes, grid, objects, 10, permille, 0)
        assert one.tolist() == [[1, 1]]
        assert np.array_equal(brute_objects_nms(scores, pairs, boxes, grid, 10, permille, 0), one)
    # a small part inside a large part's footprint: gone under one limit of 0.3, kept with a cross limit of its own
    boxes = np.int32([[0, 0, 39, 39], [10, 10, 29, 29]])  # 1600 and 400 pixels: I / U = 0.25
    assert objects_nms(scores, pairs, boxes, grid, objects, 10, 300, 200).tolist() == [[1, 1]]
    assert objects_nms(scores, pairs, boxes, grid, objects, 10, 300, 250).tolist() == [[1, 1], [0, 1]]


def test_a_tie_on_score_and_point_goes_to_the_lower_pair():
    boxes = np.int32([[0, 0, 3, 3]] * 4)
    objects = np.array([1, 0, 1, 0])  # object 0 holds pairs 1 and 3, object 1 pairs 0 and 2
    scores = np.full((2, 1, 2), 0.5, dtype=np.float32)
    pairs = np.int32([[[3, 1]], [[2, 0]]])
    grid = (0, 0, 2, 1, 10, 10)
    got = objects_nms(scores, pairs, boxes, grid, objects, 10, 1000, 1000)
    # order (bits, g, u): g = 0 holds pairs 3 (object 0) and 2 (object 1); g = 1 holds 1 and 0
    assert got.tolist() == [[1, 0], [0, 0], [1, 1], [0, 1]]
    assert np.array_equal(brute_objects_nms(scores, pairs, boxes, grid, 10, 1000, 1000), got)
    # with cross = 0 the lower pair of each point wins it and removes the other
    assert objects_nms(scores, pairs, boxes, grid, objects, 10, 1000, 0).tolist() == [[1, 0], [1, 1]]


@pytest.mark.parametrize("seed", range(6))
def test_one_object_is_nms_ref(seed):
    scores, pairs, boxes, grid, _ = _random_case(seed, G=1)
    objects = np.zeros(5, dtype=np.int64)
    for permille in (0, 300, 1000):
        for cross in (0, 1000):
            for md in (4096, 4):
                got = objects_nms(scores, pairs, boxes, grid, objects, md, permille, cross)
                want = nms_ref.nms_ref(scores[0], pairs[0], boxes, grid, md, permille)[0]
                assert (got[:, 0] == 0).all() and np.array_equal(got[:, 1], want)


@pytest.mark.parametrize("seed", range(6))
def test_relabelling_changes_nothing(seed):
    scores, pairs, boxes, grid, objects = _random_case(seed)
    perm = np.array([2, 0, 1])  # old label -> new label
    inv = np.argsort(perm)
    s2, p2, o2 = scores[inv], pairs[inv], perm[objects]
    for permille, cross in [(300, 600), (0, 1000), (1000, 0)]:
        a = objects_nms(scores, pairs, boxes, grid, objects, 4096, permille, cross)
        b = objects_nms(s2, p2, boxes, grid, o2, 4096, permille, cross)
        assert np.array_equal(perm[a[:, 0]], b[:, 0]) and np.array_equal(a[:, 1], b[:, 1])


def test_the_planes_are_the_gated_best_map_per_object():
    """objects_best: plane o is gated_best of object o's templates alone, pairs numbered in the whole set; objects_winner drops
    an entry whose unrestricted best pair fails, where objects_best keeps the next pair that passes."""
    rng = np.random.default_rng(5)
    T, A, ny, nx = 6, 2, 4, 5
    objects = np.array([2, 0, 1, 0, 1, 0])
    lens = [np.float32(rng.uniform(1, 3, size=n)) for n in (0, 2, 3, 1, 2, 4)]
    tl = np.array([l.sum(dtype=np.float32) for l in lens], dtype=np.float32)
    q = rng.choice(np.float32([0.1, 0.2, 0.2, 0.7, np.nan]), size=(T, A, ny, nx)).astype(np.float32)
    ml = (rng.uniform(0, 1, size=(T, A, ny, nx)).astype(np.float32) * tl.reshape(-1, 1, 1, 1)).astype(np.float32)
    mm = np.float32([0.5, 0.0, 0.3, 0.9])
    s, p, fr = objects_best(q, ml, objects, 4, mm, lens, skip=[0])
    assert s.shape == (4, ny, nx) and np.isnan(s[2]).all() and (p[2] == -1).all()  # object 2: only the template without lines
    assert np.isnan(s[3]).all() and np.isnan(fr[3]).all()                           # object 3: no template
    for o in (0, 1):
        idx = [t for t in range(T) if objects[t] == o]
        so, po, fo = gated_best(q[idx], ml[idx], float(mm[o]), [lens[t] for t in idx], skip=[])
        back = np.where(po >= 0, np.array(idx)[np.maximum(po, 0) // A] * A + po % A, -1)
        assert s[o].tobytes() == so.tobytes() and np.array_equal(p[o], back) and fr[o].tobytes() == fo.tobytes()
    sw, pw = objects_winner(q, ml, objects, 4, mm, lens, skip=[0])
    assert sw[1].tobytes() == s[1].tobytes() and np.array_equal(pw[1], p[1])  # min_matched 0: the gates agree
    assert not ((pw[0] >= 0) & (pw[0] != p[0])).any() and ((pw[0] < 0) & (p[0] >= 0)).any()
