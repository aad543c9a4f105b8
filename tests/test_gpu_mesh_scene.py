"""The mesh templates end to end (include/fdcm.h, "Templates from a mesh"; README, "Templates from a mesh"): templates of a
notched L-prism over 24 view_rotations, a scene that is view 7's lines turned by 30 degrees and moved, the dense detector over
36 angles, and the record read back into a 3-D rotation.  First on the CPU, with a numpy chamfer sum as the score volume and
the detector's numpy statement (tests/detect_ref.py) on a small map: view 7 at 30 degrees is the unique minimum, so the
device test asks for something the views decide."""
import os

import numpy as np
import pytest

import detect_ref as DR
import mesh_cases as MC
import mesh_ref as MR

N_VIEWS, PLANTED, ANGLE_INDEX = 24, 7, 3
ANGLES = np.deg2rad(np.arange(0, 360, 10))
CS = np.stack([np.cos(ANGLES), np.sin(ANGLES)], axis=1).astype(np.float32)


def planted_scene(template, shift):
    """(4, N) lines: the template turned by 30 degrees about the origin with the detector's float32 (c, s), then moved."""
    c, s = CS[ANGLE_INDEX]
    x1, y1, x2, y2 = template
    t = np.float32(shift[0]), np.float32(shift[1])
    return np.stack([(c * x1 + -s * y1) + t[0], (s * x1 + c * y1) + t[1], (c * x2 + -s * y2) + t[0], (s * x2 + c * y2) + t[1]])


def _points(lines, step=0.5):
    """Points every `step` pixels along (4, N) lines, and how many each line got (its weight: its length)."""
    out = []
    for x1, y1, x2, y2 in np.asarray(lines, dtype=np.float64).T:
        n = max(2, int(np.ceil(np.hypot(x2 - x1, y2 - y1) / step)) + 1)
        t = np.linspace(0.0, 1.0, n)
        out.append(np.stack([x1 + t * (x2 - x1), y1 + t * (y2 - y1)], axis=1))
    return np.concatenate(out)


def test_view_7_is_the_unique_minimum_on_the_cpu():
    """A small map (12 pixels per unit): the chamfer sum of every (view, angle) at every admissible translation, normalised
    by the number of points, through detect_ref: the first detection is view 7 at 30 degrees at the planted translation, and
    the best pose of every other pair costs at least three times as much and 0.5 pixels more."""
    import openfdcm_amd as O
    v, f = MC.notched_prism()
    views = O.view_rotations(N_VIEWS)
    mesh = MR.Mesh(v, f, MC.COS30)
    tmpls = [MR.view_lines(mesh, R, np.float32(12.0), MR.default_depth_tol(v), 2.0).T for R in views]
    assert all(t.shape[1] >= 8 for t in tmpls)
    shift = (40, 36)
    scene = planted_scene(tmpls[PLANTED], shift)
    sp = _points(scene)
    margin = 4
    ox, oy = np.floor(sp.min(axis=0)).astype(int) - margin
    W, H = (np.ceil(sp.max(axis=0)).astype(int) + margin + 1) - (ox, oy)
    yy, xx = np.mgrid[0:H, 0:W]
    D = np.sqrt(((xx[..., None] + ox - sp[:, 0]) ** 2 + (yy[..., None] + oy - sp[:, 1]) ** 2).min(axis=2))
    grid = (int(ox) - 30, int(oy) - 30, int(W) + 60, int(H) + 60, 1, 1)
    q = np.full((N_VIEWS, len(CS), grid[3], grid[2]), np.nan, dtype=np.float32)
    for t, tm in enumerate(tmpls):
        p = _points(tm)
        for a, (c, s) in enumerate(CS.astype(np.float64)):
            r = np.stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1]], axis=1)
            lo, hi = r.min(axis=0), r.max(axis=0)
            # the integer translations that keep every point on the map
            tx = np.arange(int(np.ceil(ox - lo[0])), int(np.floor(ox + W - 1 - hi[0])) + 1)
            ty = np.arange(int(np.ceil(oy - lo[1])), int(np.floor(oy + H - 1 - hi[1])) + 1)
            if not len(tx) or not len(ty):
                continue
            ix = np.rint(r[None, :, 0] + tx[:, None]).astype(int) - ox
            iy = np.rint(r[None, :, 1] + ty[:, None]).astype(int) - oy
            cost = D[iy[:, None, :], ix[None, :, :]].mean(axis=2)
            q[t, a, ty[0] - grid[1]:ty[-1] - grid[1] + 1, tx[0] - grid[0]:tx[-1] - grid[0] + 1] = cost
    rec = DR.detect_ref(q, 1, 2, 2, grid, CS)
    assert len(rec) == 1 and rec["tmpl_idx"][0] == PLANTED
    tr = rec["transform"][0]
    assert (tr[0], tr[3]) == (CS[ANGLE_INDEX][0], CS[ANGLE_INDEX][1]) and (tr[2], tr[5]) == shift
    flat = q.reshape(N_VIEWS * len(CS), -1)
    best = np.where(np.isnan(flat).all(axis=1), np.inf, np.nanmin(np.where(np.isnan(flat), np.inf, flat), axis=1))
    mine = best[PLANTED * len(CS) + ANGLE_INDEX]
    others = np.delete(best, PLANTED * len(CS) + ANGLE_INDEX)
    assert mine < 0.3 and others.min() > 3 * mine and others.min() > mine + 0.5, (mine, others.min(), int(np.argmin(others)))
    rot, pos = O.record_rotations(rec, views)
    assert np.abs(rot[0] - MC.rot("z", 30.0) @ views[PLANTED].astype(np.float64)).max() <= 1e-6 and pos[0].tolist() == list(shift)


SCALE, SHIFT = 37.3, (180, 150)


@pytest.mark.gpu
def test_detector_finds_the_planted_view():
    """View 7 of 24 at 30 degrees and exactly the planted translation is the first detection, and the unique minimum of the
    library's own score volume.

    The scale is chosen: the chamfer score of this library (the reference's evaluate) is no distance sum along the template
    line.  A line costs |I(p2) - I(p1)|, I being the integral of the distance transform along the chain of the line's
    orientation key, read at the two end points cast to int; a line leaves that chain by up to 3 degrees (depth 30), so a
    line of 200 pixels costs about 190 at the planted pose itself, and the normalised score there is 1.2, not 0.  The bowl
    round the pose is shallow (its neighbours cost 1.22 and 1.23 here), and where its bottom lies depends on the fractions
    of the end points: at 40 px per unit the library's minimum is (+1, 0) from the planted translation (1.216 against 1.430
    at the pose), at 50 px per unit (+2, -1); at 37.3 it is the pose.  Integer shifts move the map with the scene and
    change nothing.  So the equality below holds for this scale, and the second half holds at any: the detections are what
    the detector's numpy statement (tests/detect_ref.py) makes of the library's score volume."""
    import __graft_entry__ as g
    import openfdcm_amd as O
    from openfdcm_amd.engine import DeviceTemplates
    if not os.path.exists(O._capi.LIB_PATH):
        g.build()
    v, f = MC.notched_prism()
    views = O.view_rotations(N_VIEWS)
    mesh = O.Mesh(v, f)
    tmpls = O.templates_from_mesh(mesh, views, SCALE)
    ref = MR.Mesh(v, f, MC.COS30)
    assert tmpls[PLANTED].T.tobytes() == MR.view_lines(ref, views[PLANTED], np.float32(SCALE), MR.default_depth_tol(v), 2.0).tobytes()
    assert len(tmpls) == N_VIEWS and all(t.shape[1] >= 8 for t in tmpls)
    scene = planted_scene(tmpls[PLANTED], SHIFT)
    fm = O.build_cpu_featuremap(scene, O.Dt3CpuParameters(depth=30, dt3Coeff=5.0, padding=1.3))
    found = O.exhaustive_detect(fm, tmpls, radius=8, k=4, angles=ANGLES, penalty=O.DefaultPenalty(), pivot=None)
    rec = found.records()
    seen = [(int(r["tmpl_idx"]), float(r["score"]), r["transform"].tolist()) for r in rec]
    assert len(rec) >= 1 and rec["tmpl_idx"][0] == PLANTED, seen
    c, s = CS[ANGLE_INDEX]
    assert rec["transform"][0].tolist() == [c, -s, SHIFT[0], s, c, SHIFT[1]], seen
    assert len(rec) == 1 or rec["score"][0] < rec["score"][1], seen
    rot, pos = O.record_rotations(found, views)
    assert np.abs(rot[0] - MC.rot("z", 30.0) @ views[PLANTED].astype(np.float64)).max() <= 1e-6
    assert pos[0].tolist() == list(SHIFT)
    assert np.abs(rot[0] @ rot[0].T - np.eye(3)).max() <= 1e-6
    # the library's score volume on a window round the pose: the planted pose is its one minimum, and the detections on the
    # window are detect_ref's, byte for byte
    dev, tset = O._device_map(fm), DeviceTemplates(tmpls)
    grid = (SHIFT[0] - 20, SHIFT[1] - 20, 41, 41, 1, 1)
    q = DR.normalised(dev.rotation_score_map(tset, grid, CS, None), tset.lengths(), 0)
    assert q.shape == (N_VIEWS, len(CS), 41, 41)
    low = np.nanmin(q)
    assert np.argwhere(q == low).tolist() == [[PLANTED, ANGLE_INDEX, 20, 20]] and low == rec["score"][0]
    want = DR.detect_ref(q, 4, 8, 8, grid, CS)
    got = O.exhaustive_detect(fm, tmpls, radius=8, k=4, angles=ANGLES, penalty=O.DefaultPenalty(), pivot=None, window=grid).records()
    assert len(want) >= 1 and got.tobytes() == want.tobytes()
    assert got[0].tobytes() == rec[0].tobytes()
