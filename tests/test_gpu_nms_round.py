"""GPU tests of the round of the greedy rule (k_nms_round<LIST, HULL, OBJ>) at the edges of its walk, through the public calls:
the split of the runs of 256 entries over at most 256 workgroups, the reduction of the partial minima by the first lanes of a
workgroup, and the list forms' ragged last run.  Byte for byte against the referees that are there:

  * the plane forms against nms_ref.detect_nms_ref, objects_ref.detect_objects_ref and hull_ref.hull_objects_nms, on the planes
    of fdcm_best_map and fdcm_best_map_objects (held to detect_ref and objects_ref by the files that came with them);
  * the list forms against list_rule below, hull_ref.hull_list_nms' rule with the entries as arrays (a box overlap for all
    entries at once, hull_ref.overlap for those whose boxes meet the winner's), which is itself held to hull_list_nms on the
    lists of 1, 255 and 257 jobs.  A job is one template at one point, so its winner's score is that template's plane of the
    object best map with an object per template.

The case: an adopted random volume of 6 slices, 176 x 544, and four templates of one to three lines, ten pixels across."""
import numpy as np
import pytest

import hull_ref as hr
from detect_all_ref import thresholded
from detect_ref import records
from nms_ref import detect_nms_ref, footprints, point_boxes
from objects_ref import detect_objects_ref, objects_thresholded
from peaks_ref import NO_KEY

pytestmark = pytest.mark.gpu

f32 = np.float32
MARGIN = 1
OBJECTS = np.array([0, 1, 2, 0], dtype=np.int32)
G = 3
NX, NY = 144, 512  # 72 sub-tiles of 16 x 64: 288 runs of 256 keys, not a multiple of the 256 workgroups
TMPLS = [np.float32([[0, 0, 9, 3], [2, 5, 8, 1]]).T.copy(), np.float32([[-4, -2, 5, 6]]).T.copy(),
         np.float32([[0, 0, 0, 7], [0, 7, 6, 7], [6, 7, 0, 0]]).T.copy(), np.float32([[-3, 4, 6, -5], [1, 1, 4, 2]]).T.copy()]


class Rect:
    """The BOX footprint as a shape of hull_ref: every row of the box full."""

    def __init__(self, box):
        self.box = tuple(int(v) for v in box)
        n = max(0, self.box[3] - self.box[1] + 1)
        self.xl, self.xr = np.zeros(n, dtype=np.int64), np.full(n, self.box[2] - self.box[0], dtype=np.int64)
        self.area = n * (self.box[2] - self.box[0] + 1)


@pytest.fixture(scope="module")
def world():
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    rng = np.random.default_rng(28)
    keys = np.linspace(-1.3, 1.3, 6).astype(np.float32)
    dev = DeviceFeatureMap.from_volume(keys, rng.uniform(0, 40.0, size=(6, 176, 544)).astype(np.float32), (2.0, 3.0))
    w = dict(dev=dev, box=DeviceTemplates(TMPLS), hull=DeviceTemplates(TMPLS, footprint="hull"))
    x0, y0, nx, ny, _, _ = dev.exhaustive_window(w["box"], 1, 1).as_tuple()
    assert nx >= NX + 16 and ny >= NY + 16, (nx, ny)
    w["grid"] = (x0 + 8, y0 + 8, NX, NY, 1, 1)  # inside every template's admissible translations
    w["boxes"] = footprints(TMPLS, None, None, MARGIN).reshape(-1, 4)
    w["shapes"] = hr.shapes(TMPLS, None, None, MARGIN)
    w["rects"] = [Rect(b) for b in w["boxes"]]
    assert any(s.area < r.area for s, r in zip(w["shapes"], w["rects"]))
    # the planes the referees run on, each computed once
    w["best"] = dev.best_map(w["box"], w["grid"], penalty=0)
    w["best_objects"] = dev.best_map_objects(w["box"], w["grid"], OBJECTS, G, penalty=0)
    w["per_template"] = dev.best_map_objects(w["box"], w["grid"], np.arange(len(TMPLS), dtype=np.int32), len(TMPLS), penalty=0)[0]
    return w


def _bytes(parts):
    return [np.ascontiguousarray(p).tobytes() for p in parts]


def _quantile(s, q):
    v = np.sort(s[~np.isnan(s)])
    return float(v[int(len(v) * q)])


def _entries_rows(w, s, p, ent, grid):
    """(records, boxes) of the entries (object, g) of planes s, p (G, ny, nx): detect_objects_ref's rows."""
    from openfdcm_amd import _capi
    rec = np.zeros(len(ent), dtype=_capi.MATCH_DTYPE)
    F = np.zeros((len(ent), 4), dtype=np.int32)
    for l, (o, g) in enumerate(ent):
        rec[l] = records(np.array([g]), s[o].reshape(-1)[[g]], p[o], 1, None, None, grid)[0]
        F[l] = point_boxes(p[o], w["boxes"], grid)[g]
    return rec, F


# ---- a key plane of one sub-tile: 4 runs, 4 workgroups, the partials reduced by 4 lanes
def test_a_plane_of_one_sub_tile(world):
    w = world
    dev = w["dev"]
    grid = w["grid"][:2] + (13, 61, 1, 1)
    s, p = dev.best_map(w["box"], grid, penalty=0)
    assert (~np.isnan(s)).sum() > 700
    for permille in (0, 300):
        want = detect_nms_ref(s, p, w["boxes"], grid, 16, permille)
        got = dev.exhaustive_detect_nms(w["box"], grid, k=16, overlap_permille=permille, margin=MARGIN, penalty=0, boxes=True)
        assert len(got[0]) >= 4 and _bytes(got) == _bytes(want)
        ent = hr.hull_objects_nms(s, p, w["shapes"], grid, 16, permille)
        got = dev.exhaustive_detect_nms(w["hull"], grid, k=16, overlap_permille=permille, margin=MARGIN, penalty=0, boxes=True)
        assert len(got[0]) >= 4 and _bytes(got) == _bytes(_entries_rows(w, s[None], p[None], ent, grid))


# ---- a key plane of 288 runs: workgroups walk one or two runs (three or four over the 864 runs of three planes)
def test_288_runs_boxes(world):
    w = world
    s, p = w["best"]
    want = detect_nms_ref(s, p, w["boxes"], w["grid"], 64, 300)
    got = w["dev"].exhaustive_detect_nms(w["box"], w["grid"], k=64, overlap_permille=300, margin=MARGIN, penalty=0, boxes=True)
    assert len(got[0]) == 64 and _bytes(got) == _bytes(want)
    assert (np.asarray(want[1])[:, 1] > w["grid"][1] + NY - 64).any()  # a detection in the plane's last row of sub-tiles


def test_288_runs_boxes_with_objects(world):
    w = world
    s, p = w["best_objects"]
    # every entry keyed (the one-line template's object holds the low end and wins all 64), then the 0.1 % best of each plane
    # (fewer than 256 entries in all: the list is every entry that survives), where every object wins and both limits decide
    for ms, md in [(np.full(G, np.inf, dtype=np.float32), 64), (np.array([_quantile(s[o], 0.001) for o in range(G)], dtype=np.float32), 256)]:
        lists = []
        for permille, cross in [(300, 100), (300, 300), (0, 1000)]:
            rec, F, _, ent = detect_objects_ref(s, p, w["boxes"], w["grid"], OBJECTS, ms, md, permille, cross)
            got = w["dev"].exhaustive_detect_objects(w["box"], w["grid"], OBJECTS, ms, G, max_detections=md, overlap_permille=permille,
                                                     cross_permille=cross, margin=MARGIN, penalty=0, boxes=True)
            assert len(rec) >= 64 and _bytes(got) == _bytes((rec, F))
            lists.append(ent.tolist())
        if md == 256:
            assert all(len(set(o for o, g in l)) == G for l in lists) and lists[0] != lists[1] != lists[2]


@pytest.mark.parametrize("objects", [False, True])
def test_288_runs_hulls(world, objects):
    """The candidates are the entries under a threshold (about 1.5 % of a plane), so that the referee's Python loop stays short."""
    w = world
    dev, grid = w["dev"], w["grid"]
    for permille, cross in [(0, 0), (300, 100)]:
        if objects:
            ms = np.array([_quantile(w["best_objects"][0][o], 0.015) for o in range(G)], dtype=np.float32)
            s, p = objects_thresholded(*w["best_objects"], ms)
            call = lambda tset: dev.exhaustive_detect_objects(tset, grid, OBJECTS, ms, G, max_detections=48, overlap_permille=permille,
                                                              cross_permille=cross, margin=MARGIN, penalty=0, boxes=True)
        else:
            thr = _quantile(w["best"][0], 0.015)
            s, p = thresholded(*w["best"], thr)
            s, p, cross = s[None], p[None], permille
            call = lambda tset: dev.exhaustive_detect_all(tset, grid, max_score=thr, max_detections=48, overlap_permille=permille,
                                                          margin=MARGIN, penalty=0, boxes=True)
        want = hr.hull_objects_nms(s, p, w["shapes"], grid, 48, permille, cross)
        box = hr.hull_objects_nms(s, p, w["rects"], grid, 48, permille, cross)
        print("hulls, objects", objects, "permille", permille, "cross", cross, "entries", int((~np.isnan(s)).sum()),
              "first difference of the BOX and HULL lists at", next((l for l in range(48) if tuple(want[l]) != tuple(box[l])), None))
        assert len(want) == 48 and want.tolist() != box.tolist()
        assert _bytes(call(w["hull"])) == _bytes(_entries_rows(w, s, p, want, grid))
        assert _bytes(call(w["box"])) == _bytes(_entries_rows(w, s, p, box, grid))


# ---- the windows' calls: lists of 1, 255, 257 and 65 537 one-point jobs
def list_rule(keys, obj, tmpl, trans, boxes, shapes, max_det, permille, cross):
    """hull_ref.hull_list_nms on arrays: keys (n,) uint64 (NO_KEY: no entry), obj, tmpl (n,), trans (n, 2); boxes (T, 4);
    shapes: per template, None for the BOX rule.  The indices of the detections in the order found."""
    F = boxes[tmpl].astype(np.int64) + np.concatenate([trans, trans], axis=1)
    area = np.array([s.area for s in shapes], dtype=np.int64)[tmpl] if shapes else (F[:, 2] - F[:, 0] + 1) * (F[:, 3] - F[:, 1] + 1)
    left = keys != NO_KEY
    out = []
    while len(out) < max_det and left.any():
        d = int(np.argmin(np.where(left, keys, NO_KEY)))
        out.append(d)
        left[d] = False
        bw = np.maximum(0, np.minimum(F[:, 2], F[d, 2]) - np.maximum(F[:, 0], F[d, 0]) + 1)
        bh = np.maximum(0, np.minimum(F[:, 3], F[d, 3]) - np.maximum(F[:, 1], F[d, 1]) + 1)
        near = np.flatnonzero(left & (bw * bh > 0))
        inter = (bw * bh)[near]
        if shapes:
            inter = np.array([hr.overlap(shapes[tmpl[i]], tuple(trans[i]), shapes[tmpl[d]], tuple(trans[d])) for i in near], dtype=np.int64)
        limit = np.where(obj[near] == obj[d], permille, cross)
        left[near[1000 * inter > limit * (area[near] + area[d] - inter)]] = False
    return out


@pytest.mark.parametrize("n_jobs", [1, 255, 257, 65537])
def test_lists_of_one_point_jobs(world, n_jobs):
    from openfdcm_amd import _capi
    w = world
    dev = w["dev"]
    x0, y0 = w["grid"][:2]
    j = np.arange(n_jobs, dtype=np.int64)
    tmpl, trans = (j % len(TMPLS)).astype(np.int64), np.stack([x0 + j % NX, y0 + j // NX], axis=1)
    jobs = np.stack([tmpl, 0 * j, 1 + 0 * j, trans[:, 0], trans[:, 1], 1 + 0 * j, 1 + 0 * j], axis=1).astype(np.int32)
    q = w["per_template"].reshape(len(TMPLS), -1)[tmpl, j]
    assert not np.isnan(q).any()
    keys = (q.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64)
    for hull in (False, True):
        for objects in (False, True):
            obj = OBJECTS[tmpl] if objects else np.zeros(n_jobs, dtype=np.int32)
            permille, cross = (300, 100) if objects else (300, 300)
            kind = w["shapes"] if hull else None
            want = list_rule(keys, obj, tmpl, trans, w["boxes"], kind, 16, permille, cross)
            if n_jobs <= 257:  # list_rule is hull_list_nms' rule
                ent = [(int(keys[i]), int(obj[i]), (w["shapes"] if hull else w["rects"])[tmpl[i]], tuple(trans[i])) for i in range(n_jobs)]
                assert want == hr.hull_list_nms(ent, 16, permille, cross)
            assert len(want) == (16 if n_jobs > 257 else 1 if n_jobs == 1 else len(want))
            rec = np.zeros(len(want), dtype=_capi.MATCH_DTYPE)
            rec["tmpl_idx"], rec["score"] = tmpl[want], q[want]
            rec["transform"] = [[1, 0, f32(tx), 0, 1, f32(ty)] for tx, ty in trans[want]]
            F = (w["boxes"][tmpl[want]].astype(np.int64) + np.concatenate([trans[want], trans[want]], axis=1)).astype(np.int32)
            tset = w["hull"] if hull else w["box"]
            kw = dict(max_detections=16, overlap_permille=permille, margin=MARGIN, penalty=0, boxes=True, job_index=True)
            if objects:
                got = dev.exhaustive_detect_windows_objects(tset, jobs, OBJECTS, float("inf"), G, cross_permille=cross, **kw)
            else:
                got = dev.exhaustive_detect_windows(tset, jobs, **kw)
            assert _bytes(got) == _bytes((rec, F, np.array(want, dtype=np.int32))), (hull, objects)
    if n_jobs > 257:  # the set's kind matters on this list
        assert list_rule(keys, 0 * tmpl, tmpl, trans, w["boxes"], None, 16, 0, 0) != list_rule(keys, 0 * tmpl, tmpl, trans, w["boxes"], w["shapes"], 16, 0, 0)
