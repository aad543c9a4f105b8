"""GPU tests of scene selection (include/fdcm.h, "Scene selection"): the accepted poses, their counts and the residual of
fdcm_scene_select equal the referee's (tests/select_ref.py on tests/coverage_ref.py: plain integers, nothing from the kernel)
byte for byte -- there is no tolerance to choose -- on the worlds of test_gpu_coverage.py with their lists of about 60 poses
(not admissible poses, empty windows, duplicates, an overlapping cluster, the 300-line template that exceeds the LDS chunk),
plain and with the 7-angle table, forwards and reversed, over the parameter sets, max_selected 1, 3 and 4096 and radius 0, 2
and 32.  Then the section's identities on device output, a list of 270 poses that crosses two batches of rounds and stops
inside the third, the edge cases, two runs byte for byte, tensors against arrays, the public call against the method, the
per-candidate composition of scene_coverage calls on the device, and a part with a bar lying in its notch end to end."""
import numpy as np
import pytest

import select_cases as SC
import test_gpu_coverage as G
from test_select_definition import composition

pytestmark = pytest.mark.gpu


def run(w, case, labels=None, **kw):
    """The device on the case's list with the device objects of the world w: (selected, counts, residual)."""
    return w.dev.scene_select(case.labels if labels is None else labels, w.tset, case.poses, case.cs, case.pv, residual=True, **kw)


def same(got, want):
    return all(np.asarray(g).dtype == v.dtype and np.asarray(g).shape == v.shape and np.asarray(g).tobytes() == v.tobytes()
               for g, v in zip(got, want))


@pytest.mark.parametrize("radius", SC.RADII)
@pytest.mark.parametrize("rot", [False, True], ids=["plain", "angles"])
@pytest.mark.parametrize("name", SC.WORLDS)
def test_selection_equals_the_referee(name, rot, radius):
    w = G.world(name, rot)
    accepted = 0
    for reverse in (False, True):
        case = SC.world(name, rot, reverse)
        assert np.array_equal(case.labels, w.labels) and len(case.tmpls) == len(w.tmpls)
        for cov, share, pix in SC.PARAMS:
            kw = dict(radius=radius, bin_tolerance=1, min_coverage=cov, min_new=share, min_pixels=pix)
            for ms in SC.MAX_SELECTED:
                want = case.select(max_selected=ms, **kw)
                got = run(w, case, max_selected=ms, **kw)
                assert same(got, want), (reverse, cov, share, pix, ms, got[0], want[0], got[1][:4], want[1][:4])
                no_res = w.dev.scene_select(case.labels, w.tset, case.poses, case.cs, case.pv, max_selected=ms, **kw)
                assert len(no_res) == 2 and same(no_res, want[:2])
            accepted += len(want[0])
    assert accepted > 24


@pytest.mark.parametrize("name,rot,reverse", [("96x80-b5-d6", False, False), ("70x37-b5-d30-bytes", True, True), ("96x80-b0-d30", True, False)])
def test_identities_on_device_output(name, rot, reverse):
    w, case = G.world(name, rot), SC.world(name, rot, reverse)

    def device_coverage(poses):
        return w.dev.scene_coverage(case.labels, w.tset, poses, case.cs, case.pv, radius=2, bin_tolerance=1, margin=5, residual=True)
    for cov, share, pix in SC.PARAMS:
        kw = dict(radius=2, bin_tolerance=1, margin=5, min_coverage=cov, min_new=share, min_pixels=pix)
        full = run(w, case, max_selected=4096, **kw)
        SC.check_identities(case, full, max_selected=4096, coverage=device_coverage, **kw)            # 1, 2, 4, 5 (device against device)
        SC.check_identities(case, full, max_selected=4096, **kw)                                      # and against the referee
        for ms in (1, 2, 3, 5):
            part = run(w, case, max_selected=ms, **kw)
            assert np.array_equal(part[0], full[0][:ms]) and np.array_equal(part[1], full[1][:ms])    # 3
    # 6: everything at its loosest: the residual is scene coverage's of the whole list
    sel, counts, res = run(w, case, radius=2, bin_tolerance=1, margin=5, min_coverage=0.0, min_new=0.0, min_pixels=1, max_selected=4096)
    c, r = w.dev.scene_coverage(case.labels, w.tset, case.poses, case.cs, case.pv, radius=2, bin_tolerance=1, margin=5, residual=True)
    assert np.array_equal(res, r) and np.all(counts[:, 2] >= 1)
    # a list twice: no copy is accepted
    twice = SC.Case(case.labels, case.depth, case.border, case.tmpls, np.concatenate([case.poses, case.poses]), case.cs, case.pv)
    assert same(run(w, twice, radius=2, bin_tolerance=1, margin=5, max_selected=4096), run(w, case, radius=2, bin_tolerance=1, margin=5,
                                                                                         max_selected=4096))


def test_a_long_list_crosses_batches_of_rounds():
    from openfdcm_amd.engine import DeviceTemplates
    w, case = G.world("96x80-b0-d30", False), SC.long_list()
    tset = DeviceTemplates(case.tmpls)
    kw = dict(bin_tolerance=case.m // 2, **SC.LONG_KW)
    assert len(case.select(min_new=0.0, min_pixels=1, max_selected=4096, **kw)[0]) > 128      # three batches of 64, a stop in the last
    for par in (dict(min_new=0.0, min_pixels=1), dict(min_new=0.0, min_pixels=3), dict(min_new=0.5)):
        for ms in (64, 65, 4096):
            want = case.select(max_selected=ms, **par, **kw)
            got = w.dev.scene_select(case.labels, tset, case.poses, max_selected=ms, residual=True, **par, **kw)
            assert same(got, want), (par, ms, len(got[0]), len(want[0]))


def test_edge_cases_select_nothing():
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    w = G.world("70x37-b5-d30", False)
    none = np.zeros((0, 4), dtype=np.int32)
    lists = {"n = 0": none, "n = 1": np.int32([[1, 0, -1000, 0]]), "no admissible pose": np.int32([[1, 0, -1000, 0], [3, 0, 0, 5000]]),
             "no window": np.int32([[0, 0, 5, 5], [1, 0, -1000, 0]])}
    for what, poses in lists.items():
        sel, counts, res = w.dev.scene_select(w.labels, w.tset, poses, residual=True)
        assert sel.shape == (0,) and sel.dtype == np.int32 and counts.shape == (0, 3) and counts.dtype == np.int32, what
        assert np.array_equal(res, w.labels), what
        assert len(w.dev.scene_select(w.labels, w.tset, poses)[0]) == 0
    one = w.poses[30:31]                                                              # n = 1, a pose that explains pixels: accepted
    sel, counts, res = w.dev.scene_select(w.labels, w.tset, one, residual=True)
    want_c, want_r, _ = w.ref(poses=one, radius=2, bin_tolerance=1, margin=2)
    assert sel.tolist() == [0] and counts.tolist() == [[want_c[0, 0], want_c[0, 1], want_c[0, 1]]] and np.array_equal(res, want_r)
    # nothing passes the static test: more pixels than any pose explains, or a share nobody reaches
    for kw in (dict(min_pixels=1 << 24), dict(min_coverage=1.0, radius=0, margin=40)):
        sel, counts, res = w.dev.scene_select(w.labels, w.tset, w.poses, residual=True, **kw)
        assert len(SC.world("70x37-b5-d30", False).select(**kw)[0]) == 0
        assert sel.shape == (0,) and counts.shape == (0, 3) and np.array_equal(res, w.labels)
    # an empty template set, an empty map
    empty_map = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    for fm, ts, poses in [(w.dev, DeviceTemplates([]), none), (empty_map, w.tset, np.int32([[0, 0, 3, 3]])),
                          (w.dev, DeviceTemplates([]), np.int32([[0, 0, 3, 3]]))]:
        sel, counts, res = fm.scene_select(w.labels, ts, poses, bin_tolerance=0, residual=True)
        assert sel.shape == (0,) and counts.shape == (0, 3) and np.array_equal(res, w.labels)


def test_refused_arguments():
    from openfdcm_amd import _capi
    w = G.world("70x37-b5-d30", False)
    with pytest.raises(_capi.FdcmError, match=r"bin_tolerance must be in \[0, m / 2\]"):
        w.dev.scene_select(w.labels, w.tset, w.poses, bin_tolerance=w.m // 2 + 1)
    with pytest.raises(_capi.FdcmError, match=r"size must be \(width \+ 2 bx, height \+ 2 by\)"):
        w.dev.scene_select(np.ascontiguousarray(w.labels[:, :-1]), w.tset, w.poses)
    with pytest.raises(_capi.FdcmError, match="tmpl is outside the template set"):
        w.dev.scene_select(w.labels, w.tset, np.int32([[len(w.tmpls), 0, 0, 0]]))
    for kw, msg in [(dict(max_selected=0), "max_selected"), (dict(max_selected=4097), "max_selected"), (dict(min_new=1.001), "min_new_permille"),
                    (dict(min_coverage=-0.001), "min_coverage_permille"), (dict(min_pixels=0), "min_pixels")]:
        with pytest.raises(_capi.FdcmError, match=msg):
            w.dev.scene_select(w.labels, w.tset, w.poses, **kw)
    assert len(w.dev.scene_select(w.labels, w.tset, w.poses, min_new=0.9996)[0]) == len(w.dev.scene_select(w.labels, w.tset, w.poses, min_new=1.0)[0])


def test_two_runs_are_byte_identical_and_coverage_is_untouched():
    for name, rot in [("96x80-b0-d30", True), ("70x37-b5-d30-bytes", False)]:
        w, case = G.world(name, rot), SC.world(name, rot)
        before = w.run(radius=2, bin_tolerance=1, margin=40, residual=True)
        first = run(w, case, radius=2, bin_tolerance=1, margin=40, min_new=0.3, max_selected=4096)
        for _ in range(3):
            assert same(run(w, case, radius=2, bin_tolerance=1, margin=40, min_new=0.3, max_selected=4096), first)
        after = w.run(radius=2, bin_tolerance=1, margin=40, residual=True)           # the sibling shares the buffers: its bytes stay
        assert same(after, before) and same(after, w.ref(radius=2, bin_tolerance=1, margin=40)[:2])


def test_tensors_and_the_public_call():
    import torch
    import openfdcm_amd as fd
    w, case = G.world("96x80-b5-d6", True), SC.world("96x80-b5-d6", True)
    kw = dict(radius=3, bin_tolerance=1, min_coverage=0.1, min_new=0.5, min_pixels=2, max_selected=40)
    want = run(w, case, **kw)
    assert same(want, case.select(**kw)) and len(want[0]) > 3
    t = torch.from_numpy(np.array(case.labels)).cuda()
    got = run(w, case, labels=t, **kw)
    assert isinstance(got[2], torch.Tensor) and got[2].device == t.device and got[2].dtype == torch.uint8 and tuple(got[2].shape) == t.shape
    assert isinstance(got[0], np.ndarray) and same((got[0], got[1], got[2].cpu().numpy()), want)
    assert np.array_equal(t.cpu().numpy(), case.labels)                                # read in place, never written
    assert same(w.dev.scene_select(t, w.tset, case.poses, case.cs, case.pv, **kw), want[:2])   # without a residual: the handle's own plane
    flat = torch.zeros((case.labels.size + 7,), dtype=torch.uint8, device="cuda")      # a view at an odd address
    v = flat[3:3 + case.labels.size].view(case.labels.shape)
    v.copy_(t)
    got = run(w, case, labels=v, **kw)
    assert same((got[0], got[1], got[2].cpu().numpy()), want)
    wide = torch.zeros((case.height, case.width + 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        run(w, case, labels=wide[:, :case.width], **kw)
    # the public call: angles, pivots and the template cache as scene_coverage takes them
    angles = np.deg2rad(G.DEGREES)
    pub = fd.scene_select(w.dev, case.labels, case.tmpls, case.poses, angles=angles, return_residual=True, **kw)
    assert same(pub, want)
    pub = fd.scene_select(w.dev, case.labels, case.tmpls, case.poses, angles=angles, **kw)
    assert len(pub) == 2 and same(pub, want[:2])
    plain_w, plain = G.world("96x80-b5-d6", False), SC.world("96x80-b5-d6", False)
    assert same(fd.scene_select(plain_w.dev, plain.labels, plain.tmpls, plain.poses, return_residual=True), plain.select())   # the defaults
    pt = fd.scene_select(plain_w.dev, t, plain.tmpls, plain.poses, return_residual=True)
    assert isinstance(pt[2], torch.Tensor) and np.array_equal(pt[2].cpu().numpy(), plain.select()[2])


def test_the_per_candidate_composition_on_the_device_selects_the_same():
    """Identity 8 with the device's scene_coverage: one call per candidate on the running residual."""
    for name, rot, kw in [("96x80-b0-d30", False, dict(min_new=0.5)), ("70x37-b5-d30-bytes", True, dict(min_coverage=0.1, min_new=0.5, min_pixels=3))]:
        w, case = G.world(name, rot), SC.world(name, rot)

        def device_coverage(labels, poses):
            return w.dev.scene_coverage(labels, w.tset, poses, case.cs, case.pv, radius=2, bin_tolerance=1, residual=True)
        want = composition(case, radius=2, bin_tolerance=1, max_selected=4096, coverage=device_coverage, **kw)
        got = run(w, case, radius=2, bin_tolerance=1, max_selected=4096, **kw)
        assert same(got, want) and len(got[0]) > 3


def test_end_to_end_a_bar_in_the_notch_of_a_part():
    import nms_ref
    import openfdcm_amd as fd
    case = SC.notch()
    boxes = nms_ref.footprints(case.tmpls).astype(np.int64)
    a, b = boxes[0, 0] + np.int64([*G.PART_AT] * 2), boxes[1, 0] + np.int64([*SC.BAR_AT] * 2)
    inter = max(0, min(a[2], b[2]) - max(a[0], b[0]) + 1) * max(0, min(a[3], b[3]) - max(a[1], b[1]) + 1)
    union = (a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - inter
    assert 1000 * inter // union == 295                                               # a box rule at overlap 0.25 drops one of the two
    img = SC.notch_frame()
    labels = fd.edge_labels(img, depth=30, threshold=60)
    assert np.array_equal(labels, case.labels)
    fm = fd.build_image_featuremap(img, threshold=60)
    for share in (0.25, 0.5, 0.75):
        want = case.select(radius=2, bin_tolerance=1, min_new=share)
        assert want[0].tolist() == [0, 2] and int((case.labels < case.m).sum()) == 184 and int((want[2] < case.m).sum()) == 10
        got = fd.scene_select(fm, labels, case.tmpls, case.poses, radius=2, bin_tolerance=1, min_new=share, return_residual=True)
        assert same(got, want)
