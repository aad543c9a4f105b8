"""CPU-only checks of openfdcm_amd.pose_windows: it reads (template, coarse angle index, integer translation) back out of
records built with rotation_ref.rot_matrix as the library builds them, centres the run on the nearest fine angle, aligns
the window to the stride, cuts the run at the table's ends and wraps it on request."""
import numpy as np
import pytest

from rotation_ref import rot_matrix


@pytest.fixture(scope="module")
def pw():
    import openfdcm_amd
    from openfdcm_amd import _capi
    return openfdcm_amd, _capi


def _cs(angles):
    a = np.asarray(angles, dtype=np.float64)
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)


def _records(capi, poses, coarse, pivots):
    cs = _cs(coarse)
    rec = np.zeros(len(poses), dtype=capi.MATCH_DTYPE)
    for q, (t, a, tx, ty) in enumerate(poses):
        px, py = (0.0, 0.0) if pivots is None else pivots[t]
        M = rot_matrix(cs[a, 0], cs[a, 1], px, py)
        rec[q] = (t, 0.25 * q, [M[0, 0], M[0, 1], M[0, 2] + np.float32(tx), M[1, 0], M[1, 1], M[1, 2] + np.float32(ty)])
    return rec


COARSE = np.deg2rad(np.arange(0, 360, 10))
FINE = np.deg2rad(np.arange(0, 360, 1))
PIVOTS = np.float32([[3.25, -7.5], [2047.3, 1999.1], [0, 0], [4000.7, 4090.9]])


def test_round_trip_of_template_angle_and_translation(pw):
    """Translations over the range of a 4096 x 4096 map, pivots up to its far corner, every coarse angle."""
    openfdcm, capi = pw
    rng = np.random.default_rng(7)
    poses = [(int(rng.integers(0, 4)), a, int(rng.integers(-4200, 4200)), int(rng.integers(-4200, 4200))) for a in range(36)
             for _ in range(8)]
    poses += [(3, 35, 4199, -4199), (1, 0, 0, 0), (3, 18, -4199, 4199)]
    for pivots in (PIVOTS, None):
        rec = _records(capi, poses, COARSE, pivots)
        jobs = openfdcm.pose_windows(rec, COARSE, FINE, pivots, 0, 0, 0)
        assert jobs.dtype == np.int32 and jobs.shape == (len(poses), 7)
        for (t, a, tx, ty), job in zip(poses, jobs):
            assert job.tolist() == [t, 10 * a, 1, tx, ty, 1, 1]
        assert openfdcm.pose_windows(openfdcm.MatchList(rec), COARSE, FINE, pivots, 0, 0, 0).tolist() == jobs.tolist()
    with pytest.raises(ValueError):
        openfdcm.pose_windows(_records(capi, [(0, 1, 0, 0)], COARSE + 0.001, None), COARSE, FINE, None, 1, 1, 1)


def test_window_and_run_around_the_pose(pw):
    openfdcm, capi = pw
    rec = _records(capi, [(0, 3, 40, -12), (2, 20, -7, 9)], COARSE, PIVOTS)
    jobs = openfdcm.pose_windows(rec, COARSE, FINE, PIVOTS, 5, 4, 2)
    assert jobs.tolist() == [[0, 25, 11, 36, -14, 9, 5], [2, 195, 11, -11, 7, 9, 5]]


def test_nearest_fine_angle_lowest_index_on_a_tie(pw):
    openfdcm, capi = pw
    coarse = np.float64([0.0, 1.0, 3.0])
    fine = np.float64([0.5, 1.5, 2.5, 3.5, 6.0])  # 1.0 is as near to 0.5 as to 1.5; 0.0 is nearest to 6.0 on the circle
    rec = _records(capi, [(0, 1, 0, 0), (0, 2, 0, 0), (0, 0, 0, 0)], coarse, None)
    jobs = openfdcm.pose_windows(rec, coarse, fine, None, 0, 1, 1)
    assert jobs[:, 1].tolist() == [0, 2, 4] and jobs[:, 2].tolist() == [1, 1, 1]
    assert abs(6.0 - 2 * np.pi) < 0.5  # (what makes index 4 the nearest to 0)


@pytest.mark.parametrize("stride,t,half,want", [
    (1, (10, -3), (2, 3), (8, -6, 5, 7)),
    (2, (10, -3), (2, 3), (8, -6, 3, 4)),    # x: 8 10 12; y: -6 -4 -2 0
    (2, (11, -3), (2, 2), (8, -6, 4, 4)),    # x: 8 .. 14 holds 9 .. 13; y: -6 .. 0 holds -5 .. -1
    (4, (5, 6), (4, 3), (0, 0, 4, 4)),       # x: 0 4 8 12 holds 1 .. 9; y: 0 .. 12 holds 3 .. 9
    ((4, 2), (5, 6), (4, 3), (0, 2, 4, 5)),
    (3, (-7, -8), (0, 1), (-9, -9, 2, 2)),   # x: -9 -6 holds -7; y: -9 -6 holds -9 .. -7
    (3, (-9, 0), (0, 0), (-9, 0, 1, 1)),
])
def test_alignment_to_the_stride(pw, stride, t, half, want):
    """Every window point is a multiple of the stride, the window holds [t - half, t + half] and no point more than needed."""
    openfdcm, capi = pw
    rec = _records(capi, [(1, 7, t[0], t[1])], COARSE, PIVOTS)
    job = openfdcm.pose_windows(rec, COARSE, FINE, PIVOTS, 1, half[0], half[1], stride=stride)[0]
    assert tuple(job[3:]) == want
    sx, sy = (stride, stride) if np.ndim(stride) == 0 else stride
    for x0, n, s, c, h in ((job[3], job[5], sx, t[0], half[0]), (job[4], job[6], sy, t[1], half[1])):
        assert x0 % s == 0 and x0 <= c - h < x0 + s and x0 + (n - 2) * s < c + h <= x0 + (n - 1) * s


def test_run_is_cut_at_the_table_ends(pw):
    openfdcm, capi = pw
    fine = np.deg2rad(np.arange(0, 90, 1))  # a table that does not close the circle
    coarse = np.deg2rad([0, 2, 45, 88, 89])
    rec = _records(capi, [(0, a, 0, 0) for a in range(5)], coarse, None)
    jobs = openfdcm.pose_windows(rec, coarse, fine, None, 3, 0, 0)
    assert jobs[:, 1:3].tolist() == [[0, 4], [0, 6], [42, 7], [85, 5], [86, 4]]
    assert np.all(jobs[:, 1] + jobs[:, 2] <= 90)
    jobs = openfdcm.pose_windows(rec, coarse, fine, None, 200, 0, 0)
    assert jobs[:, 1:3].tolist() == [[0, 90]] * 5


def test_wrap(pw):
    openfdcm, capi = pw
    rec = _records(capi, [(0, 0, 0, 0), (0, 35, 0, 0), (0, 18, 0, 0)], COARSE, None)
    jobs = openfdcm.pose_windows(rec, COARSE, FINE, None, 5, 0, 0, wrap=True)
    assert jobs[:, 1:3].tolist() == [[355, 11], [345, 11], [175, 11]]
    assert (jobs[1, 1] + jobs[1, 2] - 1) % 360 == 355  # ends before the table's end: no crossing needed
    jobs = openfdcm.pose_windows(rec, COARSE, FINE, None, 400, 0, 0, wrap=True)
    assert np.all(jobs[:, 2] == 360) and np.all((jobs[:, 1] >= 0) & (jobs[:, 1] < 360))
    without = openfdcm.pose_windows(rec, COARSE, FINE, None, 5, 0, 0)
    assert without[:, 1:3].tolist() == [[0, 6], [345, 11], [175, 11]]
