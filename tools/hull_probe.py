#!/usr/bin/env python3
"""The case of the hull footprints' GPU tests (tests/test_gpu_hull.py) and a probe of it: the detection calls on a hull set
over a small adopted volume, digested, so that fresh processes under the tests' switches (FDCM_POISON) can be compared.

    python tools/hull_probe.py            one line per call: hull_probe <call> <sha256 of its outputs> <records>

The case: an adopted random volume of 6 slices, 96 x 160; eight templates of 0 to 6 lines, elongated so that their boxes are
mostly empty when turned (a one-line template and one without lines among them); a table of 8 rotations, 45 degrees apart;
three objects; pose-window jobs around random grid points."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

f32 = np.float32
DEPTH, WIDTH, HEIGHT, TOP = 6, 96, 160, 40.0
SEED = 77
LINES = [3, 1, 0, 6, 2, 4, 5, 2]
OBJECTS = [0, 1, 2, 0, 1, 2, 0, 1]
G = 3
MD = 4096


def cs_table():
    a = np.deg2rad(np.arange(8) * 45.0)
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)


def templates(seed=SEED):
    """Template t: its end points in an ellipse of half axes (18, 4 + t / 2) about (3 t, 2 t), turned by 20 t degrees."""
    rng = np.random.default_rng(seed)
    out = []
    for t, n in enumerate(LINES):
        p = rng.uniform(-1, 1, size=(2, 2 * n)) * np.array([[18.0], [4.0 + t / 2]])
        if n == 1:  # the one-line template: a long line, the thinnest shape there is
            p = np.array([[-17.0, 16.5], [-2.5, 3.0]])
        a = np.deg2rad(20.0 * t)
        p = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]) @ p + np.array([[3.0 * t], [2.0 * t]])
        out.append(np.ascontiguousarray(p.astype(np.float32).reshape(4, n, order="F")))
    return out


def pivots(tmpls):
    out = np.zeros((len(tmpls), 2), dtype=np.float32)
    for t, tm in enumerate(tmpls):
        if tm.shape[1]:
            xs, ys = np.concatenate([tm[0], tm[2]]), np.concatenate([tm[1], tm[3]])
            out[t] = [(xs.min() + xs.max()) / f32(2), (ys.min() + ys.max()) / f32(2)]
    return out


def volume(seed=SEED, width=WIDTH, height=HEIGHT):
    rng = np.random.default_rng(seed + 2)
    keys = np.linspace(-1.3, 1.3, DEPTH).astype(np.float32)
    return keys, rng.uniform(0, TOP, size=(DEPTH, width, height)).astype(np.float32), (2.0, 3.0)


def line_caps(tmpls):
    """A line's cost is about its length times the volume's mean, TOP / 2: with that as tau about half the lines are matched."""
    return TOP / 2


def jobs(grid, n_rot, tmpls, seed=SEED):
    """Rows (tmpl, a0, na, x0, y0, nx, ny): per template 30 windows of 3 x 3 points and 3 rotations (a run that may wrap)
    about random grid points, and two one-point jobs; the template without lines gets its jobs too."""
    rng = np.random.default_rng(seed + 3)
    x0, y0, nx, ny, sx, sy = grid
    out = []
    for t in range(len(tmpls)):
        for q in range(32):
            i, j = int(rng.integers(nx)), int(rng.integers(ny))
            a0 = int(rng.integers(n_rot))
            if q < 30:
                out.append((t, a0, min(3, n_rot), x0 + i * sx - sx, y0 + j * sy - sy, 3, 3))
            else:
                out.append((t, a0, 1, x0 + i * sx, y0 + j * sy, 1, 1))
    return np.array(out, dtype=np.int32)


def case(rot=True, stride=(1, 1)):
    """dict: dev, tmpls, caps, cs, piv (None without rotations), grid, jobs, obj."""
    from openfdcm_amd.engine import DeviceFeatureMap, DeviceTemplates
    tmpls = templates()
    dev = DeviceFeatureMap.from_volume(*volume())
    cs, piv = (cs_table(), pivots(tmpls)) if rot else (None, None)
    probe = DeviceTemplates(tmpls)
    grid = (dev.exhaustive_rotations_window(probe, cs, piv, *stride) if rot else dev.exhaustive_window(probe, *stride)).as_tuple()
    return dict(dev=dev, tmpls=tmpls, caps=line_caps(tmpls), cs=cs, piv=piv, grid=grid, stride=stride,
                jobs=jobs(grid, 8 if rot else 1, tmpls), obj=np.array(OBJECTS, dtype=np.int32))


def _quantile(s, quantile):
    v = np.sort(s[~np.isnan(s)])
    return float(v[int(len(v) * quantile)]) if len(v) else 0.0


def threshold(c, tset, quantile=0.05):
    """A score under which about `quantile` of the best map's points lie.  (On an adopted random volume a line's cost does
    not grow with its length, so the templates of one or two lines hold the low end of the single best map; the objects'
    planes, each with a threshold of its own, are where the larger templates are detected.)"""
    return _quantile(c["dev"].best_map(tset, c["grid"], c["cs"], c["piv"], penalty=0)[0], quantile)


def object_thresholds(c, tset, quantile=0.04):
    """Per object the same for its plane of the object best map."""
    s = c["dev"].best_map_objects(tset, c["grid"], c["obj"], G, c["cs"], c["piv"], penalty=0)[0]
    return np.array([_quantile(s[o], quantile) for o in range(G)], dtype=np.float32)


def calls(c, tset, thr, ms, margin=2, permille=300):
    """{name: outputs} of the detection calls that honour the set's kind.  thr: the threshold of the calls without objects;
    ms: one per object.  The windows' jobs hold few poses each: their calls get no threshold, or the objects' doubled."""
    dev, grid, cs, piv = c["dev"], c["grid"], c["cs"], c["piv"]
    sx, sy = c["stride"]
    mm = np.array([0.0, 0.4, 0.2], dtype=np.float32)
    out = {}
    out["nms"] = dev.exhaustive_detect_nms(tset, grid, cs, piv, k=16, overlap_permille=permille, margin=margin, penalty=0, boxes=True)
    for gate in ("winner", "all"):
        out["all_" + gate] = dev.exhaustive_detect_all(tset, grid, cs, piv, max_score=thr, max_detections=MD, overlap_permille=permille,
                                                       margin=margin, penalty=0, boxes=True, min_matched=0.4, matched=True, gate=gate)
        out["objects_" + gate] = dev.exhaustive_detect_objects(tset, grid, c["obj"], ms, G, cs, piv, max_detections=MD,
                                                               overlap_permille=permille, cross_permille=permille // 3, margin=margin,
                                                               penalty=0, min_matched=mm, boxes=True, matched=True, gate=gate)
        out["windows_" + gate] = dev.exhaustive_detect_windows(tset, c["jobs"], cs, piv, sx=sx, sy=sy, wrap=True, max_detections=MD,
                                                               overlap_permille=permille, margin=margin, penalty=0, min_matched=0.4, boxes=True, matched=True, job_index=True, gate=gate)
    out["windows_objects"] = dev.exhaustive_detect_windows_objects(tset, c["jobs"], c["obj"], ms * f32(2), G, cs, piv, sx=sx, sy=sy, wrap=True,
                                                                   max_detections=MD, overlap_permille=permille,
                                                                   cross_permille=permille // 3, margin=margin, penalty=0, min_matched=mm,
                                                                   boxes=True, matched=True, job_index=True, gate="all")
    return out


def digest(parts):
    h = hashlib.sha256()
    for p in parts:
        a = np.ascontiguousarray(p)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def main():
    from openfdcm_amd.engine import DeviceTemplates
    for rot, stride in [(True, (2, 3)), (False, (1, 1))]:
        c = case(rot, stride)
        tset = DeviceTemplates(c["tmpls"], line_caps=c["caps"], footprint="hull")
        for name, parts in calls(c, tset, threshold(c, tset), object_thresholds(c, tset)).items():
            print("hull_probe", name + ("_rot" if rot else ""), digest(parts), len(parts[0]), flush=True)


if __name__ == "__main__":
    main()
