"""GPU tests of scene coverage (include/fdcm.h, "Scene coverage"): the counts and the residual of fdcm_scene_coverage equal the
referee's (tests/coverage_ref.py: plain integers, nothing from the kernel) byte for byte -- there is no tolerance to choose --
on label images of 96 x 80 and 70 x 37 at border 0 and 5 and depth 6 and 30, on a hand-made image with the bytes m .. 254, with
templates of 0, 1, 3 and 40 lines, one of 300 lines (more than the kernel's LDS chunk of 256 segments), one with a zero-length
line, one whose window is the image and one whose window is a pixel wide; poses inside the image, cut by each border, wholly
outside, not admissible, duplicated and overlapping, with and without a table of 7 angles.  Then the identities on device
output, two runs byte for byte, tensors against arrays, n = 0, the refused maps, one frame end to end, and the pose-list calls
of coverage and selection under the poison in fresh processes (tools/coverage_probe.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import coverage_ref as CR
import edge_ref

pytestmark = pytest.mark.gpu

# (width, height, border, depth, kind)
WORLDS = {"96x80-b0-d30": (96, 80, 0, 30, "edges"), "96x80-b5-d6": (96, 80, 5, 6, "edges"), "70x37-b0-d6": (70, 37, 0, 6, "edges"),
          "70x37-b5-d30": (70, 37, 5, 30, "edges"), "70x37-b5-d30-bytes": (70, 37, 5, 30, "bytes")}
RADII = (0, 2, 32)
DEGREES = [0, 20, 45, 90, 135, 250, 330]
CS7 = np.stack([np.cos(np.deg2rad(DEGREES)), np.sin(np.deg2rad(DEGREES))], axis=1).astype(np.float32)


def make_labels(width, height, depth, kind, seed=3):
    m = len(edge_ref.keys_of(depth))
    if kind == "edges":
        return edge_ref.edge_labels(edge_ref.synthetic_image(width, height, seed), depth, 60)
    rng = np.random.default_rng(seed)   # hand-made: a third edges, a third the bytes m .. 254, which are no edge, the rest 255
    r = rng.uniform(size=(height, width))
    return np.where(r < 0.33, rng.integers(0, m, size=r.shape), np.where(r < 0.66, rng.integers(m, 255, size=r.shape), 255)).astype(np.uint8)


def make_templates(width, height, seed=17):
    rng = np.random.default_rng(seed)

    def lines(n, ex, ey):
        return np.stack([rng.uniform(0, ex, n), rng.uniform(0, ey, n), rng.uniform(0, ex, n), rng.uniform(0, ey, n)]).astype(np.float32)
    zero = lines(3, 20, 16)
    zero[2:, 1] = zero[:2, 1]                                                      # a zero-length line
    span = np.float32([[0.5, 0.5, width - 1.5, height - 1.5], [0.5, height - 1.5, width - 1.5, 0.5]]).T   # its window is the image
    thin = np.float32([[3.25], [1.0], [3.25], [min(height - 4.0, 20.5)]])          # vertical: its window at margin 0 is a pixel wide
    return [np.zeros((4, 0), dtype=np.float32), lines(1, 6, 5), lines(3, 24, 18), lines(40, 30, 24), lines(300, 34, 26), zero, span, thin]


def make_poses(width, height, border, n_rot, thin_x, seed=29):
    """About 60 poses (tmpl, a, x, y): random ones over the map, hand-placed ones at the borders, duplicates, a cluster.  thin_x:
    the image column the one-pixel window goes to."""
    rng = np.random.default_rng(seed)
    T = 8
    p = [[rng.integers(0, T), rng.integers(0, n_rot), rng.integers(-border - 3, width - 8), rng.integers(-border - 3, height - 6)]
         for _ in range(30)]
    p += [[6, 0, 0, 0], [7, 0, thin_x - 3, 0], [7, 0, width - 5, 2], [0, 0, 5, 5]]              # the image, a pixel wide (twice), no lines
    p += [[1, 0, -border, 3], [1, 0, 3, -border], [1, 0, width + border - 7, 3], [1, 0, 3, height + border - 6]]   # the short line at each border
    p += [[2, 0, -border, 7], [2, 0, 9, -border], [3, 0, width - 31 + border, 4], [3, 0, 5, height - 25 + border]]
    p += [[1, 0, -1000, 0], [3, 0, 0, 5000], [4, 0, width, 0], [2, n_rot - 1, (1 << 24) - 1, 0]]   # not admissible
    p += [[3, 0, 20 + i, 6 + j] for i, j in [(0, 0), (1, 0), (0, 2), (3, 3), (0, 0)]]             # overlapping windows, a duplicate
    p += [[4, n_rot - 1, 12, 5], [4, 0, 12, 5], [4, 0, 14, 4], [5, 0, 30, 10], [5, n_rot // 2, 33, 12]]
    p += [p[3], p[7], p[31]]                                                                        # duplicates
    return np.asarray(p, dtype=np.int32)


class World:
    def __init__(self, name, rot):
        from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
        import openfdcm_amd as fd
        self.width, self.height, self.border, self.depth, kind = WORLDS[name]
        self.labels = make_labels(self.width, self.height, self.depth, kind)
        self.labels.setflags(write=False)
        self.keys = edge_ref.keys_of(self.depth)
        self.m = len(self.keys)
        self.dev = DeviceFeatureMap.build_labels(self.labels, border=self.border, depth=self.depth)
        assert np.array_equal(self.dev.keys, self.keys) and (self.dev.width, self.dev.height) == (self.width + 2 * self.border,
                                                                                                  self.height + 2 * self.border)
        self.tmpls = make_templates(self.width, self.height)
        self.tset = DeviceTemplates(self.tmpls)
        self.cs = CS7 if rot else None
        self.pv = fd.template_pivots(self.tmpls) if rot else None
        self.thin_rows = slice(1, int(self.tmpls[7][3, 0]) + 1)                       # the rows of the thin template's window at y = 0
        self.thin_x = int(np.argmax((self.labels[self.thin_rows] < self.m).sum(axis=0)))   # the column with most edges in them
        self.poses = make_poses(self.width, self.height, self.border, 7 if rot else 1, self.thin_x)

    def ref(self, poses=None, labels=None, **kw):
        return CR.coverage(self.labels if labels is None else labels, self.keys, (self.border, self.border), self.dev.width, self.dev.height,
                           self.tmpls, self.poses if poses is None else poses, self.cs, self.pv, **kw)

    def run(self, poses=None, labels=None, **kw):
        return self.dev.scene_coverage(self.labels if labels is None else labels, self.tset, self.poses if poses is None else poses,
                                       self.cs, self.pv, **kw)


@functools.lru_cache(maxsize=None)
def world(name, rot):
    return World(name, rot)


def test_the_pose_lists_hold_the_cases():
    for name in WORLDS:
        for rot in (False, True):
            w = world(name, rot)
            counts, _, _ = w.ref(radius=2, bin_tolerance=1, margin=0)
            adm = counts[:, 0] >= 0
            assert 55 <= len(counts) <= 70 and adm.sum() >= 15 and (~adm).sum() >= 4, (name, rot, adm.sum())
            if not rot:
                assert w.ref(radius=2, bin_tolerance=1, margin=2)[0][30][0] == int((w.labels < w.m).sum())   # the window is the image
                thin = int((w.labels[w.thin_rows, w.thin_x] < w.m).sum())
                assert counts[31][0] == thin and thin > 0                                         # a pixel wide
                assert np.any(adm & (counts[:, 0] == 0))                                          # an empty window (or no edges in it)
            assert np.any(counts[adm, 1] > 0)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("rot", [False, True], ids=["plain", "angles"])
@pytest.mark.parametrize("name", list(WORLDS))
def test_counts_and_residual_equal_the_referee(name, rot, radius):
    w = world(name, rot)
    for tol in (0, 1, w.m // 2):
        for margin in sorted({0, radius, 40}):
            want_c, want_r, _ = w.ref(radius=radius, bin_tolerance=tol, margin=margin)
            got_c, got_r = w.run(radius=radius, bin_tolerance=tol, margin=margin, residual=True)
            assert got_c.dtype == np.int32 and got_c.shape == want_c.shape and got_r.dtype == np.uint8
            bad = np.flatnonzero((got_c != want_c).any(axis=1))
            assert bad.size == 0, (tol, margin, bad[:5], got_c[bad[:5]], want_c[bad[:5]], w.poses[bad[:5]])
            assert got_r.tobytes() == want_r.tobytes(), (tol, margin, np.argwhere(got_r != want_r)[:5])
            assert np.array_equal(w.run(radius=radius, bin_tolerance=tol, margin=margin), want_c)   # without the residual


def test_margin_none_is_the_radius_and_the_public_call():
    import openfdcm_amd as fd
    w = world("96x80-b5-d6", True)
    want = w.run(radius=3, bin_tolerance=1, margin=3)
    assert np.array_equal(w.run(radius=3, bin_tolerance=1), want)
    angles = np.deg2rad(DEGREES)
    got_c, got_r = fd.scene_coverage(w.dev, w.labels, w.tmpls, w.poses, angles=angles, radius=3, return_residual=True)
    assert np.array_equal(got_c, want) and np.array_equal(got_r, w.ref(radius=3, bin_tolerance=1, margin=3)[1])
    plain = world("96x80-b5-d6", False)
    assert np.array_equal(fd.scene_coverage(plain.dev, plain.labels, plain.tmpls, plain.poses), plain.ref(radius=2, bin_tolerance=1, margin=2)[0])


@pytest.mark.parametrize("name,rot", [("96x80-b5-d6", False), ("70x37-b5-d30-bytes", True)])
def test_identities_on_device_output(name, rot):
    w = world(name, rot)
    rng = np.random.default_rng(2)
    base = None
    for radius in (0, 1, 2, 7, 32):
        prev = None
        for tol in range(0, w.m // 2 + 1, max(1, w.m // 6)):
            c = w.run(radius=radius, bin_tolerance=tol, margin=5)
            adm = c[:, 0] >= 0
            assert np.all(c[adm, 1] <= c[adm, 0]) and np.all(c[~adm] == -1)
            if prev is not None:
                assert np.all(c[:, 1] >= prev[:, 1]) and np.array_equal(c[:, 0], prev[:, 0])
            prev = c
        if base is not None:
            assert np.all(prev[:, 1] >= base[:, 1]) and np.array_equal(prev[:, 0], base[:, 0])
        base = prev
    other = np.where(w.labels < w.m, rng.integers(0, w.m, size=w.labels.shape), w.labels).astype(np.uint8)
    a, ra = w.run(radius=2, bin_tolerance=w.m // 2, residual=True)
    b, rb = w.run(labels=other, radius=2, bin_tolerance=w.m // 2, residual=True)
    assert np.array_equal(a, b) and np.array_equal(ra == 255, rb == 255)
    h = len(w.poses) // 2
    c1, r1 = w.run(poses=w.poses[:h], residual=True)
    c2, r2 = w.run(poses=w.poses[h:], residual=True)
    c, r = w.run(residual=True)
    assert np.array_equal(c, np.concatenate([c1, c2])) and np.array_equal(r, np.where((r1 == 255) | (r2 == 255), 255, w.labels))
    cd, rd = w.run(poses=np.concatenate([w.poses, w.poses]), residual=True)
    assert np.array_equal(cd, np.concatenate([c, c])) and np.array_equal(rd, r)
    none = np.full(w.labels.shape, 255, dtype=np.uint8)
    none[::7, ::5] = w.m
    none[3::11, 2::9] = 254
    c0, r0 = w.run(labels=none, residual=True)
    assert np.all(c0[c[:, 0] >= 0] == 0) and np.array_equal(c0 < 0, c < 0) and np.array_equal(r0, none)


def test_two_runs_are_byte_identical():
    for name, rot in [("96x80-b0-d30", True), ("70x37-b5-d30-bytes", False)]:
        w = world(name, rot)
        first = w.run(radius=2, bin_tolerance=1, margin=40, residual=True)
        for _ in range(3):
            again = w.run(radius=2, bin_tolerance=1, margin=40, residual=True)
            assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()


def test_tensors_in_and_out_match_arrays():
    import torch
    w = world("70x37-b0-d6", True)
    want_c, want_r = w.run(radius=2, bin_tolerance=1, margin=40, residual=True)
    t = torch.from_numpy(np.array(w.labels)).cuda()
    got_c, got_r = w.run(labels=t, radius=2, bin_tolerance=1, margin=40, residual=True)
    assert isinstance(got_r, torch.Tensor) and got_r.device == t.device and got_r.dtype == torch.uint8 and tuple(got_r.shape) == w.labels.shape
    assert np.array_equal(got_c, want_c) and np.array_equal(got_r.cpu().numpy(), want_r)
    assert np.array_equal(t.cpu().numpy(), w.labels)                                  # read in place, never written
    assert np.array_equal(w.run(labels=t, radius=2, bin_tolerance=1, margin=40), want_c)
    # a view at an odd address: the kernel's dword loads align themselves, and never read outside the view's bytes' words
    flat = torch.full((w.labels.size + 7,), 0, dtype=torch.uint8, device="cuda")
    for off in (1, 2, 3):
        v = flat[off:off + w.labels.size].view(w.labels.shape)
        v.copy_(t)
        got_c, got_r = w.run(labels=v, radius=2, bin_tolerance=1, margin=40, residual=True)
        assert np.array_equal(got_c, want_c) and np.array_equal(got_r.cpu().numpy(), want_r)
    wide = torch.zeros((w.height, w.width + 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        w.run(labels=wide[:, :w.width])


def test_no_poses_and_empty_sets():
    from openfdcm_amd.engine import DeviceTemplates
    w = world("70x37-b5-d30", False)
    c, r = w.run(poses=np.zeros((0, 4), dtype=np.int32), residual=True)
    assert c.shape == (0, 2) and c.dtype == np.int32 and np.array_equal(r, w.labels)
    assert w.run(poses=np.zeros((0, 4), dtype=np.int32)).shape == (0, 2)
    c, r = w.dev.scene_coverage(w.labels, DeviceTemplates([]), np.zeros((0, 4), dtype=np.int32), residual=True)
    assert c.shape == (0, 2) and np.array_equal(r, w.labels)
    from openfdcm_amd.engine import DeviceFeatureMap
    empty_map = DeviceFeatureMap.from_volume(np.zeros(1, dtype=np.float32), np.zeros((1, 0, 0), dtype=np.float32), (0.0, 0.0))
    for fm, ts in [(empty_map, w.tset), (w.dev, DeviceTemplates([]))]:                 # the counts stay unwritten, as with the siblings
        c, r = fm.scene_coverage(w.labels, ts, np.int32([[0, 0, 3, 3], [0, 0, 4, 4]]), bin_tolerance=0, residual=True)
        assert np.array_equal(c, np.zeros((2, 2), dtype=np.int32)) and np.array_equal(r, w.labels)
    only = np.int32([[0, 0, 5, 5], [1, 0, -1000, 0]])                                # poses without a window alone: no launch
    c, r = w.run(poses=only, residual=True)
    assert [tuple(v) for v in c] == [(0, 0), (-1, -1)] and np.array_equal(r, w.labels)


def test_refused_maps_and_arguments():
    from openfdcm_amd import _capi, synthetic
    from openfdcm_amd.engine import DeviceFeatureMap
    w = world("70x37-b5-d30", False)
    lines_map = DeviceFeatureMap.build(synthetic.scene(96, 20, 4), depth=30, coeff=5.0, padding=1.3)
    assert np.any(lines_map.scene_translation != np.floor(lines_map.scene_translation))
    with pytest.raises(_capi.FdcmError, match="scene translation must be whole non-negative pixels"):
        lines_map.scene_coverage(w.labels, w.tset, w.poses)
    with pytest.raises(_capi.FdcmError, match=r"size must be \(width \+ 2 bx, height \+ 2 by\)"):
        w.dev.scene_coverage(np.ascontiguousarray(w.labels[:, :-1]), w.tset, w.poses)
    with pytest.raises(_capi.FdcmError, match=r"bin_tolerance must be in \[0, m / 2\]"):
        w.run(bin_tolerance=w.m // 2 + 1)
    with pytest.raises(_capi.FdcmError, match="tmpl is outside the template set"):
        w.run(poses=np.int32([[len(w.tmpls), 0, 0, 0]]))
    assert np.array_equal(w.run(bin_tolerance=w.m // 2, radius=32, margin=4096), w.ref(bin_tolerance=w.m // 2, radius=32, margin=4096)[0])


# ------------------------------------------------------------------------------------------------ end to end
PART = np.float32([[0, 0], [40, 0], [40, 14], [16, 14], [16, 34], [0, 34]])   # an L-shaped part, in its own frame
PART_AT = (18, 44)
PATCH = (92, 14, 152, 106)                                                    # x0, y0, x1, y1 of the patch of strokes


def part_template():
    nxt = np.roll(PART, -1, axis=0)
    return np.ascontiguousarray(np.concatenate([PART, nxt], axis=1).T, dtype=np.float32)


def frame():
    """160 x 120: the part alone on the left, a patch of short random strokes on the right."""
    img = np.full((120, 160), 60, dtype=np.uint8)
    x0, y0 = PART_AT
    img[y0:y0 + 14, x0:x0 + 40] = 200
    img[y0 + 14:y0 + 34, x0:x0 + 16] = 200
    rng = np.random.default_rng(8)
    for _ in range(170):
        cx, cy = rng.uniform(PATCH[0] + 4, PATCH[2] - 4), rng.uniform(PATCH[1] + 4, PATCH[3] - 4)
        ang, half = rng.uniform(0, np.pi), rng.uniform(2.0, 4.5)
        for s in np.linspace(-half, half, 24):
            img[int(round(cy + s * np.sin(ang))), int(round(cx + s * np.cos(ang)))] = 200
    return img


def in_patch(pose):
    cx, cy = pose[2] + 20, pose[3] + 17
    return PATCH[0] <= cx <= PATCH[2] and PATCH[1] <= cy <= PATCH[3]


def ratio(c):
    return c[1] / max(1, c[0])


def test_end_to_end_part_against_clutter_and_the_next_round():
    import openfdcm_amd as fd
    img, tm = frame(), part_template()
    depth, kw = 30, dict(radius=2, bin_tolerance=1)
    keys = edge_ref.keys_of(depth)
    # the referee alone, on the CPU's labels: the part's pose explains most of its window, no pose in the patch explains much
    cpu_labels = edge_ref.edge_labels(img, depth, 60)
    grid = np.int32([[0, 0, x, y] for x in range(PATCH[0] - 20, PATCH[2] - 20, 3) for y in range(PATCH[1] - 17, PATCH[3] - 17, 3)
                     if x + 40 < 160 and 0 <= y and y + 34 < 120])
    c_part = CR.coverage(cpu_labels, keys, (0, 0), 160, 120, [tm], np.int32([[0, 0, *PART_AT]]), **kw)[0][0]
    c_patch = CR.coverage(cpu_labels, keys, (0, 0), 160, 120, [tm], grid, **kw)[0]
    worst = max(ratio(c) for c in c_patch)
    assert ratio(c_part) > 0.8 and worst < 0.4 and c_part[0] > 100 and min(c[0] for c in c_patch) > 100, (c_part, worst)
    # the device: the same labels, the map, the detections on the part and in the patch
    labels = fd.edge_labels(img, depth=depth, threshold=60)
    assert np.array_equal(labels, cpu_labels)
    fm = fd.build_image_featuremap(img, threshold=60)
    dets = fd.exhaustive_detect_all(fm, [tm], float("inf"), overlap=0.3, max_detections=12)
    poses = fd.record_poses(dets)
    assert np.array_equal(poses[:, :2], np.zeros((len(poses), 2), dtype=np.int32))
    scores = dets.records()["score"]
    part = [q for q in range(len(poses)) if abs(poses[q, 2] - PART_AT[0]) <= 1 and abs(poses[q, 3] - PART_AT[1]) <= 1]
    patch = [q for q in range(len(poses)) if in_patch(poses[q])]
    assert len(part) == 1 and part[0] == 0 and patch, poses
    counts, residual = fd.scene_coverage(fm, labels, [tm], poses, return_residual=True, **kw)
    want_c, want_r, _ = CR.coverage(labels, keys, (0, 0), 160, 120, [tm], poses, **kw)
    assert np.array_equal(counts, want_c) and np.array_equal(residual, want_r)
    assert all(ratio(counts[part[0]]) > ratio(counts[q]) for q in patch), counts
    assert ratio(counts[part[0]]) > 0.8 and max(ratio(counts[q]) for q in patch) < 0.4
    # explain the part away and detect again at the score the patch's detection had: the part's pose is gone
    thr = 1.05 * float(max(scores[part[0]], scores[patch[0]]))
    c1, res1 = fd.scene_coverage(fm, labels, [tm], poses[part], return_residual=True, **kw)
    assert np.array_equal(res1, CR.coverage(labels, keys, (0, 0), 160, 120, [tm], poses[part], **kw)[1]) and c1[0, 1] == counts[part[0], 1]
    before = fd.record_poses(fd.exhaustive_detect_all(fm, [tm], thr, overlap=0.3, max_detections=12))
    assert any(np.array_equal(p, poses[part[0]]) for p in before) and any(np.array_equal(p, poses[patch[0]]) for p in before)
    fd._device_map(fm).rebuild_labels(res1)
    after = fd.record_poses(fd.exhaustive_detect_all(fm, [tm], thr, overlap=0.3, max_detections=12))
    assert not any(abs(p[2] - PART_AT[0]) <= 2 and abs(p[3] - PART_AT[1]) <= 2 for p in after), after
    assert any(in_patch(p) for p in after)


# ---- the pose-list calls in fresh processes, under the poison (tools/coverage_probe.py)
def _probe(env):
    probe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "coverage_probe.py")
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FDCM_")}
    out = subprocess.run([sys.executable, probe], capture_output=True, text=True, timeout=240, env={**clean, **env})
    assert out.returncode == 0, out.stdout + out.stderr
    return [l for l in out.stdout.splitlines() if l.startswith("coverage_probe ")][-1].split()


def test_pose_list_calls_under_the_poison_in_fresh_processes():
    """tools/coverage_probe.py -- scene_coverage and scene_select on host and device labels, with and without a residual, plain
    and with angles -- in fresh processes, one after another, each under its own time limit: the default run, FDCM_POISON=0 and
    FDCM_POISON=1 print one digest.  Nothing is started after a failure (an assertion ends the test).  The case holds what it
    is for: poses that are not admissible, windows without an edge pixel, and a selection of more than the 64 rounds of a batch."""
    want = _probe({})
    lists = int(want[9]) // 6                                     # (6 calls per list of 294 poses, 5 of them placed off the map)
    assert lists == 12 and int(want[3]) <= (294 - 5) * lists and int(want[5]) > 0 and int(want[7]) > 64, want
    for env in ({"FDCM_POISON": "0"}, {"FDCM_POISON": "1"}):
        assert _probe(env) == want, env
