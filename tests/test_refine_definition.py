"""CPU-only: the referee of fdcm_matches_refine (tests/refine_ref.py) against itself and against match_ref, on
match_cases.adopted_volume() and match_cases.record_list(77, ..): its array-wide scores are match_ref.costs_of and
pyoracle.eigen_sum pose by pose; rot = None with hx = hy = 0 is match_ref.verify's s; a wider window never raises a score;
with the centre in the table the refined score is at most s(r); permuting the list permutes the output.  Then the conditions
that keep the device tests from hiding a failure, on both maps (the line-built one from the oracle here, from the device
there), asserted before any GPU run."""
import functools

import numpy as np
import pytest

import match_cases as MC
import match_ref as R
import refine_cases as RC
import refine_ref as RR
from oracle import pyoracle as P

f32 = np.float32


@functools.lru_cache(maxsize=None)
def world(name="adopted"):
    if name == "adopted":
        keys, vol, t = MC.adopted_volume()
        base = 5
    else:
        from oracle import oracle as O
        from openfdcm_amd import synthetic
        orc = O.build(synthetic.scene(90, 24, 11), depth=12, coeff=5.0, padding=1.3, distance=O.L2, nthreads=2)
        keys, vol, t, base = orc.keys, orc.volume(), orc.translation, 0
    tmpls = MC.template_set()
    recs = MC.record_list(77, vol.shape[1], vol.shape[2], t, tmpls, 700, base)
    return keys, vol, t, tmpls, recs, base


@functools.lru_cache(maxsize=None)
def refined(name, n, na, hx, hy, sx, sy, centred=True, caps="none"):
    keys, vol, t, tmpls, recs, base = world(name)
    cs = RC.table(na, centred)
    return RR.refine(vol, keys, t, tmpls, recs[:n], base, cs=cs, pivots=RC.centre_pivots(tmpls), centre=RC.centre_of(cs), hx=hx, hy=hy,
                     sx=sx, sy=sy, caps=MC.caps_of(tmpls, caps))


def test_eigen_sum_rows_is_eigen_sum():
    rng = np.random.default_rng(2)
    for n in (0, 1, 3, 4, 7, 8, 9, 12, 16, 33, 65, 130):
        c = (rng.random((5, n)) * 30).astype(np.float32)
        if n > 2:
            c[1, 2], c[2, n - 1] = np.nan, np.inf
        assert MC.same_floats(RR.eigen_sum_rows(c), np.array([P.eigen_sum(r) for r in c], dtype=np.float32)), n


def test_the_window_is_costs_of_and_eigen_sum_pose_by_pose():
    keys, vol, t, tmpls, recs, base = world()
    caps = R.flat_caps(tmpls, MC.caps_of(tmpls, "mixed"))
    cs = RC.table(3, True)
    sets = RR.run_lines(tmpls, cs, RC.centre_pivots(tmpls))
    seen = 0
    for r in (1, 2, 10, 11, 26, 27, 43, 75):
        ti = int(recs[r]["tmpl_idx"]) - base
        if not 0 <= ti < len(tmpls) or tmpls[ti].shape[1] == 0:
            continue
        for e in (0, 2):
            p = R.posed(sets[e], recs[r], base)
            s, adm = RR.window(vol, keys, t, p, caps[ti], 2, 3, 2, 1)
            for jj in range(7):
                for ii in range(5):
                    a, v = RR.pose_score(vol, keys, t, p, caps[ti], ((ii - 2) * 2, jj - 3))
                    assert a == adm[jj, ii] and (not a or MC.same_floats(s[jj, ii:ii + 1], np.array([v], dtype=np.float32)))
                    seen += int(a)
    assert seen > 100


@pytest.mark.parametrize("caps", MC.CAPS)
def test_no_table_and_no_window_is_verify(caps):
    keys, vol, t, tmpls, recs, base = world()
    kinds = MC.caps_of(tmpls, caps)
    s = R.verify(vol, keys, t, tmpls, recs, base, kinds)[0]
    for centre in (0, -1):
        out, poses, _ = RR.refine(vol, keys, t, tmpls, recs, base, centre=centre, caps=kinds)
        lines = np.array([0 <= int(r["tmpl_idx"]) - base < len(tmpls) and tmpls[int(r["tmpl_idx"]) - base].shape[1] > 0 for r in recs])
        want = np.where(lines, s, RR.NAN).astype(np.float32)          # (a template without lines has s = +0 and no winner)
        assert MC.same_floats(out["score"], want)
        assert MC.same_floats(out["transform"], recs["transform"]) and np.array_equal(out["tmpl_idx"], recs["tmpl_idx"])
        won = ~np.isnan(want)
        assert np.all(poses[won] == (0, 0, 0)) and np.all(poses[~won] == (-1, 0, 0)) and won.sum() > 300 and (~won).sum() > 100


def test_a_wider_window_never_raises_a_score():
    small, _, _ = refined("adopted", 257, 3, 1, 1, 1, 1)
    wide, _, _ = refined("adopted", 257, 3, 2, 3, 1, 1)
    both = ~np.isnan(small["score"]) & ~np.isnan(wide["score"])
    assert both.sum() > 100 and np.all(wide["score"][both] <= small["score"][both])
    assert (wide["score"][both] < small["score"][both]).sum() > 20


@pytest.mark.parametrize("caps", ("none", "mixed"))
def test_with_the_centre_in_the_table_the_score_is_at_most_s(caps):
    keys, vol, t, tmpls, recs, base = world()
    s = R.verify(vol, keys, t, tmpls, recs[:257], base, MC.caps_of(tmpls, caps))[0]
    out, poses, _ = refined("adopted", 257, 3, 1, 1, 1, 1, True, caps)
    has = ~np.isnan(s) & np.array([tmpls[int(r["tmpl_idx"]) - base].shape[1] > 0 if 0 <= int(r["tmpl_idx"]) - base < len(tmpls) else False
                                   for r in recs[:257]])
    assert has.sum() > 100 and np.all(out["score"][has] <= s[has])
    stay = has & np.all(poses == (1, 0, 0), axis=1)
    assert MC.same_floats(out["score"][stay], s[stay]) and MC.same_floats(out["transform"][stay][:, [0, 1, 3, 4]], recs["transform"][:257][stay][:, [0, 1, 3, 4]])


def test_permuting_the_list_permutes_the_output():
    keys, vol, t, tmpls, recs, base = world()
    out, poses, _ = refined("adopted", 257, 3, 1, 1, 1, 1)
    perm = np.random.default_rng(8).permutation(257)[:90]
    cs = RC.table(3, True)
    got, gp, _ = RR.refine(vol, keys, t, tmpls, recs[:257][perm], base, cs=cs, pivots=RC.centre_pivots(tmpls), centre=RC.centre_of(cs), hx=1, hy=1)
    assert MC.same_records(got, out[perm]) and np.array_equal(gp, poses[perm])


@pytest.mark.parametrize("name", ("lines", "adopted"))
def test_the_list_meets_the_conditions_of_the_device_tests(name):
    """Of the first 257 records at the window (na, hx, hy) = (3, 2, 9): at least half have a winner, at least 10 a window that is
    only partly admissible, at least 20 no winner, at least a third of the winners are not the centre pose."""
    na, hx, hy, sx, sy = RC.CHECK_WINDOW
    out, poses, partial = refined(name, 257, na, hx, hy, sx, sy)
    RC.check_conditions(out, poses, partial, RC.centre_of(RC.table(na, True)))
