"""The experiment of tests/test_gpu_mesh_scene.py with pinhole templates (include/fdcm.h, "Templates from a mesh: pinhole views";
README, "Pinhole views"): templates of the notched prism over 24 view_rotations, the camera 5 bounding-box diagonals away, a
scene that is view 7's lines turned by 30 degrees and moved by (180, 150), the dense detector over 36 angles, and the record
read back into a pose in the camera's frame.  The same scene against orthographic templates of the same size on the image
(scale = focal / distance) is printed, not asserted: it shows what the perspective is worth at this range."""
import os

import numpy as np
import pytest

import mesh_cam_cases as CC
import mesh_cam_ref as CR
import mesh_cases as MC
import mesh_ref as MR
from test_gpu_mesh_scene import ANGLE_INDEX, ANGLES, CS, N_VIEWS, PLANTED, SCALE, SHIFT, planted_scene

DIAGONALS = 5.0


@pytest.mark.gpu
def test_detector_finds_the_planted_pinhole_view():
    """View 7 of 24 at 30 degrees is the first detection, its translation within 2 px of the planted one: the largest offset
    the README records for the bottom of this score's bowl (tests/test_gpu_mesh_scene.py says why the bowl is shallow: a line
    costs the difference of two reads of an integral, at end points cast to int).  The pose read from it puts the mesh origin
    on the detection's pixel and turns view 7 by 30 degrees."""
    import __graft_entry__ as g
    import openfdcm_amd as O
    if not os.path.exists(O._capi.LIB_PATH):
        g.build()
    v, f = MC.notched_prism()
    views = O.view_rotations(N_VIEWS)
    distance = DIAGONALS * CC.diagonal(v)
    focal = SCALE * distance                    # the size on the image of the orthographic test's templates
    positions = O.view_positions(N_VIEWS, distance)
    mesh = O.Mesh(v, f)
    tmpls = O.templates_from_mesh(mesh, views, focal=focal, positions=positions)
    ref = CR.view_lines(MR.Mesh(v, f, MC.COS30), views[PLANTED], positions[PLANTED], np.float32(focal), CR.default_near(v),
                        MR.default_depth_tol(v), 2.0)
    assert tmpls[PLANTED].T.tobytes() == ref.tobytes()
    # (the last view looks along the prism's plate from 1.2 degrees above it: at this range the rays to the plate's far side
    # pass below it, and the view keeps 7 lines of the orthographic 17)
    assert len(tmpls) == N_VIEWS and all(t.shape[1] >= 1 for t in tmpls) and tmpls[PLANTED].shape[1] >= 8
    scene = planted_scene(tmpls[PLANTED], SHIFT)
    fm = O.build_cpu_featuremap(scene, O.Dt3CpuParameters(depth=30, dt3Coeff=5.0, padding=1.3))
    found = O.exhaustive_detect(fm, tmpls, radius=8, k=4, angles=ANGLES, penalty=O.DefaultPenalty(), pivot=None)
    rec = found.records()
    seen = [(int(r["tmpl_idx"]), float(r["score"]), r["transform"].tolist()) for r in rec]
    print("pinhole templates:", seen)
    assert len(rec) >= 1 and rec["tmpl_idx"][0] == PLANTED, seen
    c, s = CS[ANGLE_INDEX]
    tr = rec["transform"][0]
    assert (tr[0], tr[1], tr[3], tr[4]) == (c, -s, s, c), seen
    assert abs(float(tr[2]) - SHIFT[0]) <= 2.0 and abs(float(tr[5]) - SHIFT[1]) <= 2.0, seen
    R_obj, T_obj = O.record_camera_poses(found, views, positions, focal)
    assert np.abs(R_obj[0] - MC.rot("z", 30.0) @ views[PLANTED].astype(np.float64)).max() <= 1e-6
    P = T_obj[0]                                 # the mesh origin under the pose
    pixel = focal * P[:2] / -P[2]
    assert np.abs(pixel - [float(tr[2]), float(tr[5])]).max() <= 1e-9 and abs(-P[2] - distance) <= 1e-4 * distance
    # what orthographic templates of the same size make of the same scene
    ortho = O.templates_from_mesh(mesh, views, SCALE)
    other = O.exhaustive_detect(fm, ortho, radius=8, k=4, angles=ANGLES, penalty=O.DefaultPenalty(), pivot=None).records()
    print("orthographic templates:", [(int(r["tmpl_idx"]), float(r["score"]), r["transform"].tolist()) for r in other])
