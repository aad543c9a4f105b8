"""One fixed set of calls with the gate inside the minimum (include/fdcm.h, "Gate inside the minimum"), for comparing the
library's paths: prints the SHA-256 of the dense records, boxes and fractions and of the windows' records, boxes, fractions
and job indices at FDCM_GATE_ALL.

    python tools/gate_probe.py                        the default path
    FDCM_MATCHED_FLAT=1 python tools/gate_probe.py    64-bit flat addresses in the dense calls by matched fraction
    FDCM_WINDOWS_FLAT=1 python tools/gate_probe.py    .. in the pose windows

The digests must be equal (tests/test_gpu_gate.py runs the switches in fresh processes: they are read once per process).
case() is also the case of that test: an adopted random volume of 4 slices of 41 x 89, twelve templates of 0 to 17 lines
whose centres lie along a diagonal (so the default window spans several 16 x 64 sub-tiles at strides (2, 3), and every
template's admissible box cuts through it), three rotations, one of them not of unit norm, and caps near the median line
cost with some +inf and one 0."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

f32 = np.float32
LINES = [0, 1, 3, 4, 7, 8, 9, 12, 13, 17, 5, 2]  # lines per template: the scalar tail alone, the trailing packet, one and
                                                 # two blocks of 8, each with and without a tail; two chunks of 8 templates
DEPTH, WIDTH, HEIGHT = 4, 41, 89
TOP = 12.0                   # the volume's values are uniform in [0, TOP): |a - b| has its median at TOP (1 - 1 / sqrt 2)
CAP = 3.5
STRIDE = (2, 3)
MIN_MATCHED = 0.5
MARGIN = 1
SEED = 2026


def cs_table():
    """Three rotations; the last one scales by 0.9."""
    a = np.array([0.0, 0.3, -0.4])
    k = np.array([1.0, 1.0, 0.9])
    return np.stack([k * np.cos(a), k * np.sin(a)], axis=1).astype(np.float32)


def templates(seed=SEED):
    rng = np.random.default_rng(seed)
    out = []
    for t, n in enumerate(LINES):
        c = np.array([2.5 * t, 13.0 * t])
        p = (c[:, None] + rng.uniform(-1, 1, size=(2, 2 * n)) * np.array([[6.0], [9.0]])).astype(np.float32).reshape(4, n, order="F")
        out.append(np.ascontiguousarray(p))
    return out


def pivots(tmpls):
    out = np.zeros((len(tmpls), 2), dtype=np.float32)
    for t, tm in enumerate(tmpls):
        if tm.shape[1]:
            xs, ys = np.concatenate([tm[0], tm[2]]), np.concatenate([tm[1], tm[3]])
            out[t] = [(xs.min() + xs.max()) / f32(2), (ys.min() + ys.max()) / f32(2)]
    return out


def line_caps(tmpls, seed=SEED):
    """Per line CAP times a factor in [0.6, 1.4]; every seventh line +inf; line 2 of template 4 has cap 0."""
    rng = np.random.default_rng(seed + 1)
    out, q = [], 0
    for t, tm in enumerate(tmpls):
        c = (CAP * rng.uniform(0.6, 1.4, size=tm.shape[1])).astype(np.float32)
        for i in range(len(c)):
            if q % 7 == 3:
                c[i] = np.inf
            q += 1
        if t == 4:
            c[2] = 0
        out.append(c)
    return out


def volume(seed=SEED, plant=False):
    """(keys, volume [k][x][y], scene translation); plant: one NaN and one +inf."""
    rng = np.random.default_rng(seed + 2)
    keys = np.linspace(-1.3, 1.3, DEPTH).astype(np.float32)
    vol = rng.uniform(0, TOP, size=(DEPTH, WIDTH, HEIGHT)).astype(np.float32)
    if plant:
        vol[1, 20, 41] = np.nan
        vol[2, 9, 60] = np.inf
    return keys, vol, (2.0, 3.0)


def build(plant=False):
    from openfdcm_amd.engine import DeviceFeatureMap
    return DeviceFeatureMap.from_volume(*volume(plant=plant))


def jobs(boxes, n_rot):
    """The job list of the windows' case, rows (tmpl, a0, na, x0, y0, nx, ny) at STRIDE.  boxes[t]: (x0, y0, nx, ny) of the
    stride-1 window of template t's admissible translations under the rotations (None without lines).  Per template with
    lines: one-point jobs, a box inside the window, boxes across its left and its upper edge, a run that wraps; then a
    duplicate and jobs on the template without lines."""
    rng = np.random.default_rng(SEED + 3)
    sx, sy = STRIDE
    out = []
    for t, b in enumerate(boxes):
        if b is None:
            out += [(t, 0, 1, 0, 0, 1, 1), (t, 1, 2, 4, 6, 3, 3)]
            continue
        x0, y0, nx, ny = b
        cx, cy = x0 + nx // 2, y0 + ny // 2
        for _ in range(3):
            out.append((t, int(rng.integers(n_rot)), 1, int(cx + rng.integers(-8, 9)), int(cy + rng.integers(-20, 21)), 1, 1))
        out.append((t, 0, n_rot, cx - 8, cy - 12, 9, 9))                  # 3 x 9 x 9, inside
        out.append((t, 2, 2, cx - 4, cy - 9, 5, 7))                       # a run that wraps: rotations 2, 0
        out.append((t, 1, 1, x0 - 5 * sx, cy - 6, 11, 5))                 # cut by the left edge
        out.append((t, 0, 2, cx - 3, y0 - 4 * sy, 4, 9))                  # cut by the upper edge
        out.append((t, 1, 2, x0 + nx - 3 * sx, y0 + ny - 2 * sy, 6, 5))   # cut by the right and the lower edge
        out.append((t, 0, 1, x0 - 9 * sx, y0 - 9 * sy, 4, 4))             # outside: no admissible point
    out.append(out[5])                                                    # a duplicate
    return np.array(out, dtype=np.int32)


def template_boxes(dev, tmpls, cs, piv):
    from openfdcm_amd.engine import DeviceTemplates
    out = []
    for t, tm in enumerate(tmpls):
        if tm.shape[1] == 0:
            out.append(None)
            continue
        g = dev.exhaustive_rotations_window(DeviceTemplates([tm]), cs, piv[t:t + 1], 1, 1).as_tuple()
        out.append(g[:4])
    return out


def case():
    """(device map, templates, caps, cs, pivots, jobs)"""
    tmpls = templates()
    cs, piv = cs_table(), pivots(tmpls)
    dev = build()
    return dev, tmpls, line_caps(tmpls), cs, piv, jobs(template_boxes(dev, tmpls, cs, piv), len(cs))


def calls(dev, tset, cs, piv, job_list):
    """The dense call with rotations at overlap 0.3 and the windows' call, both at FDCM_GATE_ALL: what the digest covers."""
    grid = dev.exhaustive_rotations_window(tset, cs, piv, *STRIDE).as_tuple()
    dense = dev.exhaustive_detect_all(tset, grid, cs, piv, max_detections=4096, overlap_permille=300, margin=MARGIN, penalty=0,
                                      boxes=True, min_matched=MIN_MATCHED, matched=True, gate="all")
    win = dev.exhaustive_detect_windows(tset, job_list, cs, piv, sx=STRIDE[0], sy=STRIDE[1], wrap=True, max_detections=4096,
                                        overlap_permille=300, margin=MARGIN, penalty=0, min_matched=MIN_MATCHED, boxes=True,
                                        matched=True, job_index=True, gate="all")
    return dense, win


def digest(parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def run():
    from openfdcm_amd.engine import DeviceTemplates
    dev, tmpls, caps, cs, piv, job_list = case()
    dense, win = calls(dev, DeviceTemplates(tmpls, line_caps=caps), cs, piv, job_list)
    return digest(dense + win), len(dense[0]) + len(win[0])


if __name__ == "__main__":
    d, n = run()
    print("gate_probe", d, "records", n)
