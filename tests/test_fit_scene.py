"""CPU-only: the planted scenes of fdcm_matches_fit (tests/fit_cases.py) on the referee (tests/fit_ref.py): an L-shaped polygon
of six lines at 12 random poses, its edges rounded to the pixel grid, 300 clutter pixels, starts off by up to 1.5 degrees and
2.5 px per axis; radius 4, bin_tolerance 2, two iterations.  The largest distance between a posed corner and the planted one
is at most 0.25 px after the fit and at most a tenth of the start's: the bound is twice the 0.118 px a float64 simulation of
the rule gave before the code was written, not a figure of the code under test.  (Measured on the referee: 0.007 .. 0.068 px
after two steps from starts of 1.1 .. 3.5 px.)  test_gpu_fit.py asks the same of the device on one of the cases."""
import numpy as np
import pytest

import fit_cases as FC


@pytest.mark.parametrize("k", range(FC.POSES))
def test_the_fit_brings_a_start_to_the_planted_pose(k):
    cases, keys, tmpls = FC.planted()
    labels, true, start = cases[k]
    assert labels.shape == (400, 400) and tmpls[0].shape == (4, 6) and int((labels < len(keys)).sum()) > 700
    before = FC.error(start["transform"][0], true)
    out, info, rms = FC.planted_fit(k)
    after = FC.error(out["transform"][0], true)
    print("case %d: start %.4f px, fitted %.4f px, pixels %d -> %d, rms %.3f -> %.3f" % (k, before, after, info[0, 2], info[0, 3], *rms[0]))
    assert info[0, 0] == 0 and info[0, 1] == 2 and info[0, 2] > 300
    assert 0.5 < before < 6.0
    assert after <= FC.MAX_ERROR and after <= FC.MAX_SHARE * before
    assert rms[0, 1] < rms[0, 0] and rms[0, 1] < 0.5         # what is left is the pixel grid's rounding
    assert out["score"][0] == start["score"][0] and out["tmpl_idx"][0] == 0
