"""CPU-only: the end-to-end scene of fdcm_matches_refine (tests/refine_cases.py) gives what test_gpu_refine.py asks of the
device.  On the oracle's own build of the scene the referee (tests/refine_ref.py), with delta_angles(2, 1 degree) and
half_x = 3, half_y = 2, returns the planted inverse pose for every perturbed record -- the true pose lies in the window of each
of the 27 -- and the score there is the unperturbed record's s."""
import numpy as np

import match_cases as MC
import match_ref as R
import refine_cases as RC
import refine_ref as RR
from oracle import oracle as O


def test_the_referee_returns_the_planted_pose():
    lines, tmpls, true, recs, planted = RC.scene()
    assert lines.shape == (4, 12) and len(recs) == 27
    orc = O.build(lines, distance=O.L2, nthreads=2, **RC.BUILD)
    vol, keys, t = orc.volume(), orc.keys, orc.translation
    s_true = R.verify(vol, keys, t, tmpls, true)[0]
    assert not np.isnan(s_true[0])
    cs = RC.cs_of((np.arange(2 * RC.HALF_STEPS + 1) - RC.HALF_STEPS) * RC.STEP)
    assert RC.centre_of(cs) == RC.HALF_STEPS
    out, poses, _ = RR.refine(vol, keys, t, tmpls, recs, cs=cs, pivots=RC.PIVOT, centre=RC.HALF_STEPS, hx=RC.HALF_X, hy=RC.HALF_Y)
    assert np.array_equal(poses, planted), np.flatnonzero(np.any(poses != planted, axis=1))
    assert np.all(out["score"] == s_true[0])
    # the refined transform is the true one up to float32 rounding of the composed rotations, far below a pixel
    assert np.abs(out["transform"] - true["transform"][0]).max() < 1e-3
    # refine_matches -> detect_matches: the refined records tie on the score and overlap, so the first, the unperturbed one, is
    # kept, and its transform is the true one as floats
    assert tuple(planted[0]) == (RC.HALF_STEPS, 0, 0)
    kept, idx, _, _ = R.detect(vol, keys, t, tmpls, out, permille=300)
    assert len(kept) == 1 and idx[0] == 0 and np.array_equal(kept["transform"][0], true["transform"][0])
    # the perturbed records as they came score worse, all but the unperturbed one
    s_in = R.verify(vol, keys, t, tmpls, recs)[0]
    moved = np.any(planted != (RC.HALF_STEPS, 0, 0), axis=1)
    assert moved.sum() == 26 and np.all(s_in[moved] > s_true[0]) and MC.same_floats(s_in[~moved], s_true)
