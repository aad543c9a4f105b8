"""The referee of scene coverage and selection of match records (tests/match_coverage_ref.py; include/fdcm.h, "Match lists:
scene coverage and selection") against the section's identities, on the referee alone: integer translations against
coverage_ref and select_ref (identity 1), scene coverage's and scene selection's identities (2, 3), the segments' end points
against the pixels the oracle's evaluate reads (4), the record lists' contents, and a case worked by hand.  No device."""
import numpy as np
import pytest

import coverage_ref as CR
import match_coverage_cases as CS
import match_coverage_ref as MC
import match_ref as MR
import select_cases as SC
import select_ref as SR
from edge_ref import keys_of
from oracle import pyoracle as P

f32 = np.float32


def same(a, b):
    return all(np.asarray(x).dtype == np.asarray(y).dtype and np.asarray(x).shape == np.asarray(y).shape
               and np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def test_a_case_worked_by_hand():
    """Depth 6: slice 0 is vertical, slice 3 horizontal.  The template is an open box, (0,0)-(4,0), (0,0)-(0,3), (4,0)-(4,3); the
    record turns it by 90 degrees, (x, y) -> (8.5 - y, 1.5 + x): the posed lines are (8.5,1.5)-(8.5,5.5), vertical, and
    (8.5,1.5)-(5.5,1.5) and (8.5,5.5)-(5.5,5.5), horizontal.  With T = (2, 2) the map pixels are (10,3)-(10,7), (10,3)-(7,3),
    (10,7)-(7,7): in the 12 x 9 label image the segments (8,1)-(8,5), (8,1)-(5,1), (8,5)-(5,5).  F(r) = [5, 1, 8, 5].
    Edge pixels (x, y: label): (8,2: 0) on the vertical segment; (9,3: 0) a pixel right of it, outside F(r) at margin 0; (6,1: 3)
    on the upper segment; (6,5: 2) on the lower one, a slice off; (6,3: 3) two pixels from both; (1,7: 3) far away; (7,3) holds
    200, no edge."""
    keys = keys_of(6)
    tm = [np.float32([[0, 0, 4], [0, 0, 0], [4, 0, 4], [0, 3, 3]])]
    rec = MR.records([0], [0], [[0, -1, 8.5, 1, 0, 1.5]])
    ok, ends, bins, _ = MC.segments(keys, (2, 2), 16, 13, tm, rec[0])
    assert ok and ends.T.tolist() == [[10, 3, 10, 7], [10, 3, 7, 3], [10, 7, 7, 7]] and bins.tolist() == [0, 3, 3]
    assert MR.footprints(tm, rec)[0].tolist() == [5, 1, 8, 5]
    lab = np.full((9, 12), 255, dtype=np.uint8)
    for (x, y), v in {(8, 2): 0, (9, 3): 0, (6, 1): 3, (6, 5): 2, (6, 3): 3, (1, 7): 3, (7, 3): 200}.items():
        lab[y, x] = v
    for (radius, tol, margin), counts, gone in [((1, 0, 1), (5, 3), [(8, 2), (9, 3), (6, 1)]),
                                                ((1, 1, 1), (5, 4), [(8, 2), (9, 3), (6, 1), (6, 5)]),
                                                ((2, 1, 1), (5, 5), [(8, 2), (9, 3), (6, 1), (6, 5), (6, 3)]),
                                                ((1, 0, 0), (4, 2), [(8, 2), (6, 1)]),
                                                ((0, 3, 0), (4, 3), [(8, 2), (6, 1), (6, 5)])]:
        c, res, _ = MC.coverage(lab, keys, (2, 2), 16, 13, tm, rec, radius=radius, bin_tolerance=tol, margin=margin)
        want = lab.copy()
        for x, y in gone:
            want[y, x] = 255
        assert c.tolist() == [list(counts)] and np.array_equal(res, want), (radius, tol, margin, c)
    # the same record twice: the second explains nothing new and is not accepted; moved off the map it is (-1, -1)
    two = np.concatenate([rec, rec, MR.records([0, 1], [0, 0], [[0, -1, 8.5, 1, 0, -3.5], [1, 0, 0, 0, 1, 0]])])
    sel, c3, res = MC.select(lab, keys, (2, 2), 16, 13, tm, two, radius=1, bin_tolerance=0, margin=1, min_new=0.0)
    assert sel.tolist() == [0] and c3.tolist() == [[5, 3, 3]]
    assert MC.coverage(lab, keys, (2, 2), 16, 13, tm, two, radius=1, bin_tolerance=0, margin=1)[0].tolist() == [[5, 3], [5, 3], [-1, -1], [-1, -1]]


@pytest.mark.parametrize("name", SC.WORLDS)
def test_identity_1_integer_translations_are_the_pose_calls(name):
    case, world = CS.pose_case(name), SC.world(name, False)
    for radius, tol, margin in [(2, 1, None), (0, 0, 40), (32, case.m // 2, 5)]:
        kw = dict(radius=radius, bin_tolerance=tol, margin=margin)
        want = world.coverage(**kw)
        got = case.coverage(**kw)
        assert same(got[:2], want[:2])
        assert all((a is None) == (b is None) and (a is None or np.array_equal(a, b)) for a, b in zip(got[2], want[2]))
        for par in (dict(min_new=0.5), dict(min_coverage=0.3, min_new=0.0, min_pixels=3, max_selected=3)):
            assert same(case.select(**kw, **par), world.select(**kw, **par))


@pytest.mark.parametrize("name", CS.WORLDS)
def test_the_record_lists_hold_the_cases(name):
    case = CS.case(name)
    recs, T = case.recs, len(case.tmpls)
    t = recs["tmpl_idx"].astype(np.int64) - case.base
    counts = case.coverage(radius=2, bin_tolerance=1)[0]
    adm = counts[:, 0] >= 0
    assert 50 <= len(recs) <= 70 and (t < 0).sum() >= 2 and (t >= T).sum() >= 2 and not adm[(t < 0) | (t >= T)].any()
    M = recs["transform"]
    assert np.isnan(M).any(axis=1).sum() >= 1 and np.isinf(M).any(axis=1).sum() >= 2 and not adm[~np.isfinite(M).all(axis=1)].any()
    valid = (t >= 0) & (t < T)
    assert (valid & (t == 0) & adm).any() and np.all(counts[valid & (t == 0) & adm] == 0)        # the template without lines
    assert (valid & (t == 4) & adm).sum() >= 2 and case.tmpls[4].shape[1] == 300                 # two LDS chunks
    rot = np.isfinite(M).all(axis=1) & (M[:, 1] != 0) & (M[:, 2] != np.rint(M[:, 2])) & (M[:, 5] != np.rint(M[:, 5]))
    assert (rot & adm).sum() >= 12
    assert (np.abs(np.hypot(M[:, 0], M[:, 3]) - np.hypot(M[:, 1], M[:, 4])) > 0.3).sum() >= 1    # a non-uniform scale
    keyed = [recs[j:j + 1].tobytes()[4:] for j in range(len(recs))]
    assert len(keyed) - len(set(keyed)) >= 4                                                     # exact duplicates
    # within a pixel of the map's sides: admissible records with an end pixel in the map's first or last column or row, and
    # records that are not admissible although every posed coordinate is within a pixel of the map
    edge_in = edge_out = 0
    for j in np.flatnonzero(valid & np.isfinite(M).all(axis=1)):
        ok, ends, _, p = MC.segments(case.keys, case.T, case.W, case.H, case.tmpls, recs[j], case.base)
        q = np.stack([p[0] + f32(case.border), p[1] + f32(case.border), p[2] + f32(case.border), p[3] + f32(case.border)])
        if ok and ends.size and (ends[[0, 2]].min() == 0 or ends[[1, 3]].min() == 0 or ends[[0, 2]].max() == case.W - 1 or ends[[1, 3]].max() == case.H - 1):
            edge_in += 1
        if not ok and q.size and q[[0, 2]].min() > -2 and q[[1, 3]].min() > -2 and q[[0, 2]].max() < case.W + 1 and q[[1, 3]].max() < case.H + 1:
            edge_out += 1
    assert edge_in >= 4 and edge_out >= 3, (edge_in, edge_out)
    if case.border:                                                                              # windows cut to a column and to nothing
        wins = [MC.window(case.tmpls, recs[j], case.base, 2, case.width, case.height) for j in np.flatnonzero(adm & (t == 7))]
        assert any(x0 == x1 == case.width - 1 and y0 <= y1 for x0, y0, x1, y1 in wins) and any(x0 > x1 for x0, y0, x1, y1 in wins)
    assert CS.BASES[name] == case.base and any(b != 0 for b in CS.BASES.values())


@pytest.mark.parametrize("name", ["96x80-b5-d6", "70x37-b5-d30-bytes"])
def test_identity_2_scene_coverages_identities_carry_over(name):
    case = CS.case(name)
    prev = None
    for radius in (0, 2, 7):
        row = None
        for tol in (0, 1, case.m // 2):
            c = case.coverage(radius=radius, bin_tolerance=tol, margin=5)[0]
            adm = c[:, 0] >= 0
            assert np.all(c[adm, 1] <= c[adm, 0]) and np.all(c[~adm] == -1)
            assert row is None or (np.array_equal(row[:, 0], c[:, 0]) and np.all(row[:, 1] <= c[:, 1]))
            row = c
        assert prev is None or np.all(prev[:, 1] <= row[:, 1])
        prev = row
    relabeled = np.where(case.labels < case.m, (case.labels.astype(np.int64) * 7 + 3) % case.m, case.labels).astype(np.uint8)
    assert np.array_equal(case.coverage(labels=relabeled, radius=2, bin_tolerance=case.m // 2)[0], case.coverage(radius=2, bin_tolerance=case.m // 2)[0])
    (ca, ra, _), (cb, rb, _), (cc, rc, _) = case.coverage(recs=case.recs[:25]), case.coverage(recs=case.recs[25:]), case.coverage()
    assert np.array_equal(np.concatenate([ca, cb]), cc) and np.array_equal(np.where((ra == 255) | (rb == 255), 255, case.labels), rc)
    blank = np.full_like(case.labels, 255)
    c, r, _ = case.coverage(labels=blank)
    assert np.all(c[c[:, 0] >= 0] == 0) and np.array_equal(r, blank)


@pytest.mark.parametrize("name", ["96x80-b0-d30", "70x37-b5-d30"])
def test_identity_3_scene_selections_identities_carry_over(name):
    case = CS.case(name)
    for cov, share, pix in SC.PARAMS:
        kw = dict(radius=2, bin_tolerance=1, margin=5, min_coverage=cov, min_new=share, min_pixels=pix)
        full = case.select(max_selected=4096, **kw)
        CS.check_identities(case, full, max_selected=4096, **kw)
        for ms in (1, 2, 5):
            part = case.select(max_selected=ms, **kw)
            assert np.array_equal(part[0], full[0][:ms]) and np.array_equal(part[1], full[1][:ms])
    # one coverage call per candidate on the running residual selects the same records
    counts = case.coverage()[0]
    running, chosen = case.labels, []
    for j in range(len(case.recs)):
        if counts[j, 1] < 1:
            continue
        c, r, _ = case.coverage(recs=case.recs[j:j + 1], labels=running)
        if c[0, 1] >= 1 and 1000 * int(c[0, 1]) >= 500 * int(counts[j, 1]):
            running, chosen = r, chosen + [j]
    got = case.select(min_new=0.5, max_selected=4096)
    assert got[0].tolist() == chosen and np.array_equal(got[2], running) and len(chosen) > 3


class Reads:
    """A volume that records where it is read: vol[k][x, y] notes (k, x, y) and is 0."""

    def __init__(self):
        self.at = []

    def __getitem__(self, k):
        at = self.at

        class Slice:
            def __getitem__(self, xy):
                at.append((int(k), int(xy[0]), int(xy[1])))
                return f32(0)
        return Slice()


@pytest.mark.parametrize("name", ["96x80-b5-d6", "70x37-b5-d30"])
def test_identity_4_the_end_points_are_the_pixels_evaluate_reads(name):
    case = CS.case(name)
    lines = 0
    for r in case.recs:
        s = MC.segments(case.keys, case.T, case.W, case.H, case.tmpls, r, case.base)
        if s is None or not s[0]:
            continue
        _, ends, bins, p = s
        for i in range(min(p.shape[1], 40)):
            one = np.ascontiguousarray(p[:, i:i + 1])                     # the one-line template {posed line i}
            vol = Reads()
            P.evaluate({"t": (f32(case.T[0]), f32(case.T[1])), "vol": vol}, one, [P.closest_orientation(case.keys, one[:, 0])], (f32(0), f32(0)))
            assert vol.at == [(int(bins[i]), int(ends[0, i]), int(ends[1, i])), (int(bins[i]), int(ends[2, i]), int(ends[3, i]))]
            assert 0 <= min(vol.at[0][1], vol.at[1][1]) and max(vol.at[0][1], vol.at[1][1]) < case.W
            lines += 1
    assert lines > 150
