"""The end-to-end case of tests/test_gpu_pyramid.py on the CPU: the numpy chain of tests/pyramid_scene.py (pyramid_ref's level
images, edge_ex_ref's labels, the oracle's volume and scores, window_detect_ref's rule) recovers the three planted poses through
the pyramid at levels 1 and 2 and through the strided coarse pass at strides 2 and 4 -- what the scene was designed to, before any
device saw it.  No GPU."""
import numpy as np
import pytest

import pyramid_scene as S


def test_the_scene_is_what_the_case_says():
    img = S.frame()
    assert img.shape == (192, 256) and img.dtype == np.uint8 and set(np.unique(img)) >= {S.BACKGROUND, S.VALUE}
    assert len(S.PLANTS) == 3 and {p[0] for p in S.PLANTS} == {0, 1} and len(S.templates()) == 2
    coarse_deg = set(np.rint(np.rad2deg(S.COARSE)).astype(int).tolist())
    assert all(p[1] not in coarse_deg for p in S.PLANTS)          # no planted angle is a coarse angle
    for shape, deg, tx, ty in S.PLANTS:                             # every part lies inside the frame
        poly = S.posed_polygon(shape, deg, tx, ty)
        assert poly.min() > 4 and poly[:, 0].max() < S.WIDTH - 4 and poly[:, 1].max() < S.HEIGHT - 4


@pytest.mark.parametrize("level,coarse_stride", [(1, 1), (2, 1), (0, 2), (0, 4)])
def test_numpy_chain_recovers_the_planted_poses(level, coarse_stride):
    dets, jobs, seeds, every = S.cpu_chain(level, coarse_stride)
    print("level", level, "stride", coarse_stride, "seeds", len(seeds), "best per job", np.round(every, 3).tolist())
    found, n = S.recovered(dets)
    assert found == [True, True, True] and n == 3
    # the threshold separates the parts from the junk with room on both sides
    assert every[2] < S.MAX_SCORE / 2 and every[3] > 2 * S.MAX_SCORE
