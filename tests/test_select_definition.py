"""The referee of scene selection (tests/select_ref.py; include/fdcm.h, "Scene selection") against a second, independent
statement of the rule -- the literal loop of one coverage_ref call per candidate on a running residual, identity 8 --, the
section's identities 1 to 6 on the referee, the round formulation of the section simulated in Python against the sequential
rule, a case worked by hand, and the facts the GPU tests build on (the long list, the part with the bar in its notch).  No
device."""
import numpy as np
import pytest

import coverage_ref as CR
import select_cases as SC
import select_ref as SR
from edge_ref import keys_of

CASES = [(name, rot) for name in SC.WORLDS for rot in (False, True)]
IDS = [f"{name}-{'angles' if rot else 'plain'}" for name, rot in CASES]


def composition(case, radius=2, bin_tolerance=1, margin=None, min_coverage=0.0, min_new=0.5, min_pixels=1, max_selected=1024,
                coverage=None):
    """Identity 8: one coverage call on the labels for the static test, then one per candidate on the running residual, whose
    `explained` is `new`.  coverage(labels, poses) -> (counts, residual): the referee's by default."""
    if coverage is None:
        def coverage(labels, poses):
            return case.coverage(poses=poses, labels=labels, radius=radius, bin_tolerance=bin_tolerance, margin=margin)[:2]
    cov, share = SR.permille(min_coverage), SR.permille(min_new)
    counts = np.asarray(coverage(case.labels, case.poses)[0])
    running = case.labels
    selected, rows = [], []
    for q in range(len(case.poses)):
        edges, explained = int(counts[q, 0]), int(counts[q, 1])
        if len(selected) == max_selected:
            break
        if edges < 0 or explained < min_pixels or 1000 * explained < cov * edges:
            continue
        c, r = coverage(running, case.poses[q:q + 1])
        new = int(c[0, 1])
        if new >= min_pixels and 1000 * new >= share * explained:
            running = r
            selected.append(q)
            rows.append((edges, explained, new))
    return np.asarray(selected, dtype=np.int32), np.asarray(rows, dtype=np.int32).reshape(-1, 3), running


def rounds(case, radius=2, bin_tolerance=1, margin=None, min_coverage=0.0, min_new=0.5, min_pixels=1, max_selected=1024):
    """The round formulation: count everything once; per accepted pose d claim E_d, recount only the surviving later candidates
    whose window meets d's, drop those that now fail; the next accepted pose is the first survivor."""
    counts, _, masks = case.coverage(radius=radius, bin_tolerance=bin_tolerance, margin=margin)
    win = case.windows(radius if margin is None else margin)
    cov, share = SR.permille(min_coverage), SR.permille(min_new)
    n = len(case.poses)
    alive = [masks[q] is not None and counts[q, 1] >= min_pixels and 1000 * int(counts[q, 1]) >= cov * int(counts[q, 0]) for q in range(n)]
    cur = [int(c) for c in counts[:, 1]]
    claimed = np.zeros(case.labels.shape, dtype=bool)
    selected, rows, recounts = [], [], 0
    d = next((q for q in range(n) if alive[q]), None)
    while d is not None and len(selected) < max_selected:
        selected.append(d)
        rows.append((int(counts[d, 0]), int(counts[d, 1]), cur[d]))
        claimed |= masks[d]
        for q in range(d + 1, n):
            if alive[q] and win[q, 0] <= win[d, 2] and win[d, 0] <= win[q, 2] and win[q, 1] <= win[d, 3] and win[d, 1] <= win[q, 3]:
                cur[q] = int((masks[q] & ~claimed).sum())
                recounts += 1
                alive[q] = cur[q] >= min_pixels and 1000 * cur[q] >= share * int(counts[q, 1])
        d = next((q for q in range(d + 1, n) if alive[q]), None)
    residual = np.where(claimed, 255, case.labels).astype(np.uint8)
    return np.asarray(selected, dtype=np.int32), np.asarray(rows, dtype=np.int32).reshape(-1, 3), residual, recounts


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))


# ------------------------------------------------------------------------------------------------ by hand
def test_a_case_worked_by_hand():
    """16 x 12, every pixel an edge of slice 3, horizontal 8-pixel segments (bin 3), radius 0: a pose explains exactly its 8
    pixels.  Poses at x = 0 (columns 0 .. 7), 0 again (a duplicate), 3 (3 .. 10: 5 of 8 claimed, 3 new), 8 (8 .. 15: 3 claimed
    by the one at 3 if that was accepted, else none), one row below (nothing claimed) and one outside the map."""
    labels = np.full((12, 16), 3, dtype=np.uint8)
    hor = np.float32([[0], [5], [7], [5]])
    poses = np.int32([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 3, 0], [0, 0, 8, 0], [0, 0, 0, 1], [0, 0, 900, 0]])
    case = SC.Case(labels, 6, 0, [hor], poses)
    assert [tuple(c) for c in case.coverage(radius=0, margin=0)[0]] == [(8, 8)] * 5 + [(-1, -1)]
    kw = dict(radius=0, margin=0)
    sel, counts, res = case.select(min_new=0.5, **kw)               # 3 of 8 is below a half; the pose at 8 keeps all 8
    assert sel.tolist() == [0, 3, 4] and counts.tolist() == [[8, 8, 8]] * 3 and (res == 255).sum() == 24
    sel, counts, res = case.select(min_new=0.375, **kw)             # 3000 >= 375 * 8: accepted; then the pose at 8 has 5 of 8 new
    assert sel.tolist() == [0, 2, 3, 4] and counts[:, 2].tolist() == [8, 3, 5, 8] and (res == 255).sum() == 24
    sel, counts, _ = case.select(min_new=0.375, min_pixels=4, **kw)
    assert sel.tolist() == [0, 3, 4] and counts[:, 2].tolist() == [8, 8, 8]
    sel, counts, _ = case.select(min_new=0.0, min_pixels=1, max_selected=2, **kw)
    assert sel.tolist() == [0, 2]
    margin = case.select(radius=0, margin=1, min_coverage=0.3)      # windows of 10 x 3 = 30 edges, or 27 where the image cuts a column
    assert len(margin[0]) == 0 and np.array_equal(margin[2], labels)   # 8 of 27 is below 0.3: nobody is a candidate
    assert case.select(radius=0, margin=1, min_coverage=0.25)[0].tolist() == [0, 3, 4]


# ------------------------------------------------------------------------------------------------ the worlds
@pytest.mark.parametrize("name,rot", CASES, ids=IDS)
def test_referee_equals_the_per_candidate_composition(name, rot):
    case = SC.world(name, rot)
    for radius, params in [(2, (0.0, 0.5, 1)), (2, (0.3, 1.0, 3)), (0, (0.0, 0.0, 1)), (32, (0.3, 0.5, 3))]:
        kw = dict(radius=radius, bin_tolerance=1, margin=radius, min_coverage=params[0], min_new=params[1], min_pixels=params[2])
        for ms in (3, 4096):
            assert same(case.select(max_selected=ms, **kw), composition(case, max_selected=ms, **kw)), (radius, params, ms)


@pytest.mark.parametrize("reverse", [False, True], ids=["list", "reversed"])
@pytest.mark.parametrize("name,rot", CASES, ids=IDS)
def test_identities_and_the_rounds_on_the_referee(name, rot, reverse):
    case = SC.world(name, rot, reverse)
    accepted = recounted = 0
    for radius in SC.RADII:
        for cov, share, pix in SC.PARAMS:
            kw = dict(radius=radius, bin_tolerance=1, margin=radius, min_coverage=cov, min_new=share, min_pixels=pix)
            full = case.select(max_selected=4096, **kw)
            SC.check_identities(case, full, max_selected=4096, **kw)                                   # 1, 2, 4, 5
            for ms in SC.MAX_SELECTED:
                part = case.select(max_selected=ms, **kw)
                assert np.array_equal(part[0], full[0][:ms]) and np.array_equal(part[1], full[1][:ms])   # 3
                got = rounds(case, max_selected=ms, **kw)
                assert same(part, got), (radius, cov, share, pix, ms)
            accepted += len(full[0])
            recounted += got[3]
    assert accepted > 100 and recounted > accepted       # the lists hold conflicts: poses are recounted, not only accepted
    # 6: everything at its loosest
    sel, counts, res = case.select(radius=2, bin_tolerance=1, margin=2, min_coverage=0.0, min_new=0.0, min_pixels=1, max_selected=4096)
    c, r, masks = case.coverage(radius=2, bin_tolerance=1, margin=2)
    assert np.array_equal(res, r)
    claimed, want = np.zeros(case.labels.shape, dtype=bool), []
    for q, mk in enumerate(masks):
        if mk is not None and (mk & ~claimed).any():
            want.append(q)
            claimed |= mk
    assert sel.tolist() == want


def test_duplicates_and_the_order_of_the_list():
    case = SC.world("96x80-b0-d30", False)
    sel, _, _ = case.select(min_new=0.0, max_selected=4096)
    twice = SC.Case(case.labels, case.depth, case.border, case.tmpls, np.concatenate([case.poses, case.poses]))
    again = twice.select(min_new=0.0, max_selected=4096)
    assert np.array_equal(again[0], sel) and np.all(again[0] < len(case.poses))      # 4: no copy of an accepted pose, nor of a refused one
    rev = SC.world("96x80-b0-d30", False, True).select(min_new=0.5, max_selected=4096)
    fwd = case.select(min_new=0.5, max_selected=4096)
    n = len(case.poses)
    assert sorted(n - 1 - rev[0]) != fwd[0].tolist()                                  # the order is the priority: it matters


# ------------------------------------------------------------------------------------------------ what the GPU tests build on
def test_the_long_list_crosses_two_batches_of_rounds():
    case = SC.long_list()
    assert len(case.poses) == 270
    kw = dict(bin_tolerance=case.m // 2, **SC.LONG_KW)
    got = {k: len(case.select(max_selected=4096, **p, **kw)[0]) for k, p in
           [("pixels1", dict(min_new=0.0, min_pixels=1)), ("pixels3", dict(min_new=0.0, min_pixels=3)), ("new", dict(min_new=0.5))]}
    assert got == {"pixels1": 154, "pixels3": 82, "new": 138}
    for p in (dict(min_new=0.0, min_pixels=1), dict(min_new=0.5)):
        for ms in (64, 65, 4096):
            assert same(case.select(max_selected=ms, **p, **kw), rounds(case, max_selected=ms, **p, **kw))


def test_the_bar_in_the_notch_of_the_part():
    import nms_ref
    case = SC.notch()
    boxes = nms_ref.footprints(case.tmpls).astype(np.int64)
    a = boxes[0, 0] + np.int64([*SC.G.PART_AT] * 2)
    b = boxes[1, 0] + np.int64([*SC.BAR_AT] * 2)
    inter = max(0, min(a[2], b[2]) - max(a[0], b[0]) + 1) * max(0, min(a[3], b[3]) - max(a[1], b[1]) + 1)
    union = (a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - inter
    assert 1000 * inter // union == 295           # the greedy box rule at overlap 0.25 drops one of the two parts
    for share in (0.25, 0.5, 0.75):
        sel, counts, res = case.select(radius=2, bin_tolerance=1, min_new=share)
        assert sel.tolist() == [0, 2], (share, sel, counts)
        # what is left is the ten corner pixels of the two outlines, whose slices are diagonal
        assert int((case.labels < case.m).sum()) == 184 and int((res < case.m).sum()) == 10
        assert same((sel, counts, res), composition(case, radius=2, bin_tolerance=1, min_new=share))
    # with no test of the new share every shifted copy that explains one pixel more is kept
    assert len(case.select(radius=2, bin_tolerance=1, min_new=0.0)[0]) > 2


def test_keys_of_the_worlds():
    assert len(keys_of(30)) == 30 and len(keys_of(6)) == 6 and CR.frame((5, 5), 106, 90, 96, 80) == (5, 5)
