"""Every call that lays out the workspace the seam and the exhaustive search share (search.eval, search.eval_stage), on one
fixed case, for comparing the library's paths and a handle's histories: prints the SHA-256 of each call's outputs.

    python tools/exhaustive_probe.py                                    the default path, order "shuffled"
    python tools/exhaustive_probe.py --order listed|reversed|shuffled|fresh
    FDCM_POISON=1 python tools/exhaustive_probe.py --threshold 0x1.8p+3  the workspace and the volume filled with a word
    FDCM_EXHAUSTIVE_FLAT=1 python tools/exhaustive_probe.py ...          64-bit flat addresses in the dense calls

One line per call, `exhaustive_probe <call name> <sha256>`, and a last line with counts.  The digests of every order and of
every switch must be equal (tests/test_gpu_workspace.py runs the switches in fresh processes: they are read once per
process).  An order runs its calls on one handle, "fresh" makes a handle per call.  --threshold: the max_score of the call
whose list ends early, as float.hex(); without it the process takes it from its own best map (the default run does, and
hands it to the others: a process under a switch must not derive its own)."""
import hashlib
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEFAULT, EXPONENTIAL = 0, 1  # the penalties (include/fdcm.h)
MAX_DET = 200

# The C entry points that reserve the shared workspace: tests/test_workspace_abi.py derives the list from the binding by
# WORKSPACE_SYMBOL and wants each in COVERED (a call of CALLS reaches it) or in EXEMPT (with the reason).
WORKSPACE_SYMBOL = re.compile(r"^fdcm_(search_exhaustive(_\w+)?|score_map(_\w+)?|best_map(_\w+)?|line_costs(_\w+)?|matched_fractions(_\w+)?|"
                              r"featuremap_evaluate(_\w+)?|featuremap_minmax_translation(_\w+)?)$")
COVERED = {
    "fdcm_featuremap_evaluate", "fdcm_featuremap_minmax_translation", "fdcm_featuremap_minmax_translation_batch",
    "fdcm_score_map", "fdcm_score_map_rotations", "fdcm_search_exhaustive", "fdcm_search_exhaustive_peaks",
    "fdcm_search_exhaustive_rotations", "fdcm_best_map", "fdcm_search_exhaustive_detect", "fdcm_search_exhaustive_detect_nms",
    "fdcm_search_exhaustive_detect_all", "fdcm_search_exhaustive_detect_all_matched", "fdcm_search_exhaustive_windows",
    "fdcm_search_exhaustive_detect_windows", "fdcm_line_costs", "fdcm_matched_fractions", "fdcm_best_map_gated",
    "fdcm_search_exhaustive_detect_all_gated", "fdcm_search_exhaustive_detect_windows_gated",
    "fdcm_best_map_objects", "fdcm_search_exhaustive_detect_objects", "fdcm_search_exhaustive_detect_windows_objects",
}
EXEMPT = {
    "fdcm_score_map_device": "fdcm_score_map's driver and workspace layout with the planes in the caller's device memory, which is "
                             "not the workspace; the probe holds no device memory of its own",
}


def case():
    """The inputs, the same in every process and without a device: matched_probe's scene, templates (0, 3, 9 and 70 lines),
    rotations and pivots; the small grids (partial 16 x 64 sub-tiles on both axes, partly outside every admissible box) and
    the large one (the workspace grows); a pose list on and around the first small grid; a handful of pose windows."""
    from openfdcm_amd import synthetic
    scene = synthetic.scene(256, 48, 9)
    rng = np.random.default_rng(67)
    tmpls = []
    for n in (0, 3, 9, 70):
        c = rng.uniform(110, 150, size=2)
        tmpls.append((c[:, None] + rng.uniform(-40, 40, size=(2, 2 * n))).astype(np.float32).reshape(4, n, order="F"))
    a = np.deg2rad([0, 45, 250])
    cs = np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)
    piv = np.float32([[0, 0], [120, 130], [128.5, 127.25], [131, 119]])
    small = [(-95, -100, 37, 70, 1, 1), (-120, -130, 37, 70, 3, 2)]
    large = (-240, -60, 200, 120, 1, 1)
    poses = {}
    for rot in (False, True):
        A = len(cs) if rot else 1
        rows = []
        for x0, y0, nx, ny, sx, sy in small:
            xs, ys = np.meshgrid(x0 + sx * np.arange(0, nx, 5), y0 + sy * np.arange(0, ny, 7))
            rows += [(t, q, x, y) for t in range(len(tmpls)) for q in range(A) for x, y in zip(xs.ravel(), ys.ravel())]
        rows += [(3, 0, 9000, 0), (1, A - 1, 0, -(1 << 24) + 1), (0, 0, 5, 5)]  # far outside the map; the template without lines
        poses[rot] = np.array(rows, dtype=np.int32)
    sizes = [(1, 1), (3, 3), (5, 2), (17, 65), (37, 70), (9, 9), (64, 16), (4, 16)]
    runs = [(0, 1), (0, 3), (2, 2), (1, 1), (1, 3), (2, 1), (0, 2), (2, 3)]
    jobs = np.array([(q % 4, runs[q][0], runs[q][1], -110 + 7 * q, -120 + 9 * q, sizes[q][0], sizes[q][1]) for q in range(8)],
                    dtype=np.int32)
    return {"scene": scene, "tmpls": tmpls, "tau": 3.0, "cs": cs, "piv": piv, "small": small, "large": large, "poses": poses,
            "jobs": jobs, "depth": 12, "padding": 1.2, "coeff": 5.0}


class Ctx:
    """What a call works with: the case, the handle, the two template sets and the threshold."""

    def __init__(self, c, dev, sets, threshold):
        self.c, self.dev, self.sets, self.threshold = c, dev, sets, threshold
        self.cs, self.piv, self.small, self.large = c["cs"], c["piv"], c["small"], c["large"]

    def rots(self):
        return [(None, None), (self.cs, self.piv)]


def _grid_points(grid):
    x0, y0, nx, ny, sx, sy = grid
    xs, ys = np.meshgrid(x0 + sx * np.arange(nx), y0 + sy * np.arange(ny))
    return np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float32)


# ---- the calls: each returns the list of every array it was handed back, and notes (records, room) of its lists
def _evaluate(x, note):
    return [s for g in x.small for s in x.dev.evaluate(x.c["tmpls"], [_grid_points(g)] * len(x.c["tmpls"]))]


def _minmax(x, note):
    tm = x.c["tmpls"]
    av = np.float32([[1, 0], [0, 1], [0.6, -0.8], [-1, 1]])
    out = [x.dev.minmax_translation_batch(tm, av), x.dev.minmax_translation_batch(tm[3:], av[:1])]
    return out + [x.dev.minmax_translation(tm[t], av[t]) for t in (1, 2, 3)]


def _score_map(x, note):
    return [x.dev.score_map(s, g) for s in x.sets for g in x.small]


def _rotation_score_map(x, note):
    return [x.dev.rotation_score_map(s, g, x.cs, x.piv) for s in x.sets for g in x.small]


def _large_maps(x, note):
    return [x.dev.score_map(x.sets[0], x.large), x.dev.rotation_score_map(x.sets[1], x.large, x.cs, x.piv)]


def _large_detect_all(x, note):
    out = []
    for s, (cs, pv) in zip(x.sets, x.rots()):
        rec, box = x.dev.exhaustive_detect_all(s, x.large, cs, pv, max_detections=MAX_DET, overlap_permille=300, margin=1,
                                               penalty=DEFAULT, boxes=True)
        note(len(rec), MAX_DET)
        out += [rec, box]
    return out


def _search(k):
    def call(x, note):
        out = []
        for s in x.sets:
            for g in x.small:
                out.append(x.dev.exhaustive_search(s, g, k=k))
                note(len(out[-1]), 3 * k)
        return out
    return call


def _peaks(x, note):
    out = []
    for s in x.sets:
        for g in x.small:
            out.append(x.dev.exhaustive_peaks(s, g, k=8, rx=8, ry=8))
            note(len(out[-1]), 3 * 8)
    return out


def _rotation_search(x, note):
    out = []
    for s in x.sets:
        for g in x.small:
            for k, rx, ry, ra, wrap in [(8, 2, 3, 1, True), (64, 0, 0, 0, False), (5, 8, 1, 1, False)]:
                out.append(x.dev.exhaustive_rotation_search(s, g, x.cs, x.piv, k=k, rx=rx, ry=ry, ra=ra, wrap=wrap))
                note(len(out[-1]), 3 * k)
    return out


def _best_map(x, note):
    out = []
    for s in x.sets:
        for g in x.small:
            for cs, pv in x.rots():
                for penalty, tau in [(None, 1.0), (EXPONENTIAL, 1.5)]:
                    out += list(x.dev.best_map(s, g, cs, pv, penalty=penalty, tau=tau))
    return out


def _detect(x, note):
    out = []
    for s in x.sets:
        for g in x.small:
            for cs, pv in x.rots():
                for k, r in [(8, 4), (64, 0)]:
                    out.append(x.dev.exhaustive_detect(s, g, cs, pv, k=k, rx=r, ry=r, penalty=DEFAULT))
                    note(len(out[-1]), k)
    return out


def _detect_nms(x, note):
    out = []
    for s in x.sets:
        for g in x.small:
            for cs, pv in x.rots():
                for k, permille in [(8, 300), (64, 1000)]:
                    rec, box = x.dev.exhaustive_detect_nms(s, g, cs, pv, k=k, overlap_permille=permille, margin=2, penalty=DEFAULT,
                                                           boxes=True)
                    note(len(rec), k)
                    out += [rec, box]
    return out


def _detect_all(at_threshold):
    def call(x, note):
        out = []
        for s in x.sets:
            for g in x.small:
                for cs, pv in x.rots():
                    # (overlap 1000 suppresses the winner alone: the list at +inf fills where the grid has MAX_DET candidates)
                    rec, box = x.dev.exhaustive_detect_all(s, g, cs, pv, max_score=x.threshold if at_threshold else float("inf"),
                                                           max_detections=MAX_DET, overlap_permille=300 if at_threshold else 1000,
                                                           margin=1, penalty=DEFAULT, boxes=True)
                    note(len(rec), MAX_DET)
                    out += [rec, box]
        return out
    return call


def _detect_all_matched(x, note):
    out = []
    for g in x.small:
        for cs, pv in x.rots():
            got = x.dev.exhaustive_detect_all(x.sets[1], g, cs, pv, max_detections=MAX_DET, overlap_permille=300, margin=1,
                                              penalty=DEFAULT, min_matched=0.4, boxes=True, matched=True)
            note(len(got[0]), MAX_DET)
            out += list(got)
    return out


def _gate_all(x, note):
    """The gate inside the minimum (include/fdcm.h): the gated best map, the dense call with and without a threshold and the
    windows' call, all at FDCM_GATE_ALL."""
    out = []
    jobs = x.c["jobs"]
    for s in x.sets:
        for cs, pv in x.rots():
            g = x.small[0]
            out += list(x.dev.best_map(s, g, cs, pv, penalty=DEFAULT, min_matched=0.4, matched=True))
            for max_score in (float("inf"), x.threshold):
                got = x.dev.exhaustive_detect_all(s, g, cs, pv, max_score=max_score, max_detections=MAX_DET, overlap_permille=300, margin=1,
                                                  penalty=DEFAULT, min_matched=0.4, boxes=True, matched=True, gate="all")
                note(len(got[0]), MAX_DET)
                out += list(got)
        got = x.dev.exhaustive_detect_windows(s, jobs, x.cs, x.piv, wrap=True, max_detections=MAX_DET, overlap_permille=300, margin=1,
                                              penalty=DEFAULT, min_matched=0.2, boxes=True, matched=True, job_index=True, gate="all")
        note(len(got[0]), MAX_DET)
        out += list(got)
    return out


def _objects(x, note):
    """Objects (include/fdcm.h): the object best map, the dense call under both gates and the windows' call, three objects
    of which one is empty, thresholds and needs per object."""
    out = []
    jobs = x.c["jobs"]
    obj, mm = [2, 0, 2, 0], [0.4, 0.0, 0.2]
    for s in x.sets:
        for cs, pv in x.rots():
            g = x.small[0]
            out += list(x.dev.best_map_objects(s, g, obj, 3, cs, pv, penalty=DEFAULT, min_matched=mm, matched=True))
            for gate, ms in (("winner", [float("inf"), 0.0, x.threshold]), ("all", float("inf"))):
                got = x.dev.exhaustive_detect_objects(s, g, obj, ms, 3, cs, pv, max_detections=MAX_DET, overlap_permille=300,
                                                      cross_permille=600, margin=1, penalty=DEFAULT, min_matched=mm, boxes=True,
                                                      matched=True, gate=gate)
                note(len(got[0]), MAX_DET)
                out += list(got)
        got = x.dev.exhaustive_detect_windows_objects(s, jobs, obj, [float("inf"), 0.0, 1e30], 3, x.cs, x.piv, wrap=True,
                                                      max_detections=MAX_DET, overlap_permille=300, cross_permille=600, margin=1,
                                                      penalty=DEFAULT, min_matched=mm, boxes=True, matched=True, job_index=True)
        note(len(got[0]), MAX_DET)
        out += list(got)
    return out


def _windows(x, note):
    out = []
    jobs = x.c["jobs"]
    for s in x.sets:
        out += list(x.dev.exhaustive_window_search(s, jobs, x.cs, x.piv, sx=1, sy=1, wrap=True, k=8))
        out += list(x.dev.exhaustive_window_search(s, [(j[0], 0, 1, j[3], j[4], j[5], j[6]) for j in jobs], sx=3, sy=2, k=4))
    return out


def _detect_windows(x, note):
    out = []
    jobs = x.c["jobs"]
    for s in x.sets:
        got = x.dev.exhaustive_detect_windows(s, jobs, x.cs, x.piv, wrap=True, max_detections=MAX_DET, overlap_permille=300, margin=1,
                                              penalty=DEFAULT, min_matched=0.2, boxes=True, matched=True, job_index=True)
        note(len(got[0]), MAX_DET)
        out += list(got)
        got = x.dev.exhaustive_detect_windows(s, [(j[0], 0, 1, j[3], j[4], j[5], j[6]) for j in jobs], sx=3, sy=2, max_detections=2,
                                              overlap_permille=1000, penalty=DEFAULT, boxes=True, job_index=True)
        out += list(got)
    return out


def _line_costs(x, note):
    out = []
    for s in x.sets:
        for rot, (cs, pv) in zip((False, True), x.rots()):
            out += list(x.dev.line_costs(s, x.c["poses"][rot], cs, pv))
    return out


def _matched_fractions(x, note):
    return [x.dev.matched_fractions(s, x.c["poses"][rot], cs, pv) for s in x.sets for rot, (cs, pv) in zip((False, True), x.rots())]


# "listed": the large grid first, so that the small calls after it run inside a large buffer that holds its leftovers
CALLS = [
    ("large_score_maps", _large_maps), ("large_detect_all", _large_detect_all), ("evaluate", _evaluate),
    ("minmax_translation", _minmax), ("score_map", _score_map), ("rotation_score_map", _rotation_score_map),
    ("exhaustive_search_k1", _search(1)), ("exhaustive_search_k64", _search(64)), ("exhaustive_peaks_r8", _peaks),
    ("exhaustive_rotation_search", _rotation_search), ("best_score_map", _best_map), ("exhaustive_detect", _detect),
    ("exhaustive_detect_nms", _detect_nms), ("exhaustive_detect_all_inf", _detect_all(False)),
    ("exhaustive_detect_all_threshold", _detect_all(True)), ("exhaustive_detect_all_matched", _detect_all_matched),
    ("exhaustive_window_search", _windows), ("exhaustive_detect_windows", _detect_windows), ("line_costs", _line_costs), ("matched_fractions", _matched_fractions),
    ("gate_all", _gate_all), ("objects", _objects),
]
NAMES = [name for name, _ in CALLS]


def orders():
    """The three orders of the call list on one handle: permutations of NAMES."""
    shuffled = [NAMES[i] for i in np.random.default_rng(2024).permutation(len(NAMES))]
    return {"listed": list(NAMES), "reversed": NAMES[::-1], "shuffled": shuffled}


def _build(c):
    from openfdcm_amd.engine import DeviceFeatureMap
    return DeviceFeatureMap.build(c["scene"], depth=c["depth"], coeff=c["coeff"], padding=c["padding"], distance=0)


def _sets(c):
    from openfdcm_amd.engine import DeviceTemplates
    return [DeviceTemplates(c["tmpls"]), DeviceTemplates(c["tmpls"], line_caps=c["tau"])]


def threshold(c=None):
    """The max_score that leaves a list shorter than MAX_DET: the 2 % quantile of the finite scores of this process's own best
    map of the first small grid (at most 52 of its 2590 points pass), on a handle of its own."""
    c = c or case()
    scores, _ = _build(c).best_map(_sets(c)[0], c["small"][0], penalty=DEFAULT)
    fin = np.sort(scores[np.isfinite(scores)])
    return float(fin[len(fin) // 50])


def run(order="shuffled", thr=None, keep=False):
    """Runs the calls in the order (a key of orders(), "fresh", or a list of names).  Returns (digests {name: sha256}, counts
    {records, finite, nan, short, full}, outputs {name: arrays} when keep).  short / full: lists that came back with fewer
    records than they had room for / with exactly MAX_DET."""
    c = case()
    if thr is None:
        thr = threshold(c)
    sets = _sets(c)
    fresh = order == "fresh"
    names = list(NAMES) if fresh else (orders()[order] if isinstance(order, str) else list(order))
    assert sorted(names) == sorted(NAMES)
    table = dict(CALLS)
    dev = None if fresh else _build(c)
    digests, outputs = {}, {}
    counts = {"records": 0, "finite": 0, "nan": 0, "short": 0, "full": 0}

    def note(n, room):
        counts["short"] += n < room
        counts["full"] += room == MAX_DET and n == MAX_DET

    for name in names:
        x = Ctx(c, _build(c) if fresh else dev, sets, thr)
        got = table[name](x, note)
        h = hashlib.sha256()
        for a in got:
            a = np.ascontiguousarray(a)
            h.update(f"{a.dtype.str}{a.shape}".encode())
            h.update(a.tobytes())
            if a.dtype.names:  # match records
                counts["records"] += len(a)
                a = np.ascontiguousarray(a["score"])
            if a.dtype == np.float32:
                counts["finite"] += int(np.isfinite(a).sum())
                counts["nan"] += int(np.isnan(a).sum())
        digests[name] = h.hexdigest()
        if keep:
            outputs[name] = got
    return digests, counts, outputs


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--order", default="shuffled", choices=["listed", "reversed", "shuffled", "fresh"])
    ap.add_argument("--threshold", default=None, help="float.hex() of the max_score of the list that ends early")
    a = ap.parse_args(argv)
    digests, counts, _ = run(a.order, None if a.threshold is None else float.fromhex(a.threshold))
    for name in NAMES:
        print(f"exhaustive_probe {name} {digests[name]}")
    print("exhaustive_probe counts " + " ".join(f"{k} {v}" for k, v in counts.items()))


if __name__ == "__main__":
    main(sys.argv[1:])
