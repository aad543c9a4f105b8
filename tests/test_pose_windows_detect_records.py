"""pose_windows reads the records of the detect family (exhaustive_detect, _nms, _all) as it reads the rotation search's:
the transform layout {c, -s, m.x + t.x, s, c, m.y + t.y} is the same and the normalised score is not looked at.  No device:
the records are written by the layout's rule (include/fdcm.h, "Best map and detections")."""
import numpy as np


def test_detect_records_give_the_jobs_of_their_poses():
    import openfdcm_amd as openfdcm
    from openfdcm_amd import _capi
    tmpls = [np.float32([[0, 0, 10, 0], [10, 0, 10, 6]]).T.copy(), np.float32([[2, 1, 9, 14]]).T.copy()]
    piv = openfdcm.template_pivots(tmpls)
    coarse = np.deg2rad(np.arange(0, 360, 30))
    fine = np.deg2rad(np.arange(0, 360, 2))
    poses = [(1, 4, 33, -7), (0, 11, -5, 120), (0, 0, 0, 0)]  # (tmpl, coarse angle, tx, ty)
    rec = np.zeros(len(poses), dtype=_capi.MATCH_DTYPE)
    for q, (t, a, tx, ty) in enumerate(poses):
        c, s = np.float32(np.cos(coarse[a])), np.float32(np.sin(coarse[a]))
        px, py = piv[t]
        ns = -s
        mx, my = px - (c * px + ns * py), py - (s * px + c * py)
        rec[q] = (t, 0.25 * q, [c, ns, mx + np.float32(tx), s, c, my + np.float32(ty)])  # a normalised score, ascending
    jobs = openfdcm.pose_windows(openfdcm.MatchList(rec), coarse, fine, piv, 3, 2, 1, wrap=True)
    assert jobs.dtype == np.int32 and jobs.tolist() == [[1, 57, 7, 31, -8, 5, 3], [0, 162, 7, -7, 119, 5, 3], [0, 177, 7, -2, -1, 5, 3]]
    assert np.array_equal(openfdcm.pose_windows(rec, coarse, coarse, piv, 0, 0, 0)[:, [0, 1, 3, 4]], np.int32(poses))
