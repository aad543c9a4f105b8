"""The cases the tests of fdcm_matches_refine share (include/fdcm.h, "Match lists: refinement").  Not collected: the tests
import it.

The windows (na, hx, hy, sx, sy) of the device tests, the delta tables and pivots they run with, and the end-to-end scene: one
template of twelve lines posed at a known transform makes the scene, and records of that template are the true pose
perturbed by every combination of (-2, 0, +2 degrees) x (-3, 0, +3 px) x (-2, 0, +2 px).  test_refine_scene.py confirms on
the CPU, with the oracle's own build and the referee, what test_gpu_refine.py then asks of the device: refine_matches with
delta_angles(2, 1 degree), half_x = 3, half_y = 2 brings every perturbed record back to the planted pose."""
import numpy as np

import match_ref as R

f32 = np.float32
WINDOWS = ((1, 0, 0, 1, 1), (3, 1, 1, 1, 1), (2, 0, 2, 1, 3), (5, 2, 0, 2, 1), (3, 2, 9, 1, 1))   # the first with rot = None
LENGTHS = (1, 3, 4, 5, 255, 256, 257)
CHECK_WINDOW = (3, 2, 9, 1, 1)     # the window at which the conditions on the list are asserted


def cs_of(angles):
    """_angles' table: float32(cos(float64)), float32(sin(float64))."""
    a = np.asarray(angles, dtype=np.float64).reshape(-1)
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)


def table(na, centred):
    """The (na, 2) delta table of a window: steps of 1.5 degrees around zero when centred (the zero exact), else beside it."""
    k = np.arange(na, dtype=np.float64) - (na // 2 if centred else -1)
    return cs_of(k * np.deg2rad(1.5))


def centre_of(cs):
    """The index whose (c, s) is exactly (1, 0), else -1."""
    unit = np.flatnonzero(np.all(np.asarray(cs, dtype=np.float32).reshape(-1, 2) == f32([1, 0]), axis=1))
    return int(unit[0]) if unit.size else -1


def centre_pivots(templates):
    """pivot "center": the centre of each template's bounding box in float32, (0, 0) without lines."""
    out = np.zeros((len(templates), 2), dtype=np.float32)
    for t, tm in enumerate(templates):
        a = np.asarray(tm, dtype=np.float32).reshape(4, -1)
        if a.shape[1]:
            xs, ys = np.concatenate([a[0], a[2]]), np.concatenate([a[1], a[3]])
            out[t] = ((xs.min() + xs.max()) / f32(2), (ys.min() + ys.max()) / f32(2))
    return out


def check_conditions(out, poses, partial, centre):
    """What keeps the device tests from hiding a failure, of the referee's result for the first 257 records at CHECK_WINDOW."""
    won = ~np.isnan(out["score"])
    assert len(out) == 257 and won.sum() >= 129, won.sum()
    assert partial.sum() >= 10, partial.sum()
    assert (~won).sum() >= 20, (~won).sum()
    moved = won & np.any(poses != (centre, 0, 0), axis=1)
    assert 3 * moved.sum() >= won.sum(), (moved.sum(), won.sum())


# ---- the end-to-end scene
PART = np.float64([[0, 0], [46, 4], [88, 0], [92, 30], [84, 62], [60, 58], [58, 84], [30, 88], [26, 60], [4, 64], [8, 40], [-2, 22]])
TRUE_POSE = (0.4, 70.0, 40.0)                       # (angle, x, y): the part rotated about its pivot, then moved
PIVOT = np.float32([[45.0, 44.0]])                  # the centre of PART's bounding box
ANGLES = np.deg2rad([-2.0, 0.0, 2.0])
SHIFTS_X, SHIFTS_Y = (-3, 0, 3), (-2, 0, 2)
HALF_STEPS, STEP, HALF_X, HALF_Y = 2, np.deg2rad(1.0), 3, 2
BUILD = dict(depth=30, coeff=5.0, padding=1.6)


def polygon_lines(pts):
    pts = np.asarray(pts, dtype=np.float64)
    return np.concatenate([pts, np.roll(pts, -1, axis=0)], axis=1).T      # (4, N): x1, y1, x2, y2


def pose_matrix(angle, x, y):
    """The float32 record transform of a rotation by angle about PIVOT followed by the translation (x, y)."""
    c, s = np.cos(angle), np.sin(angle)
    px, py = float(PIVOT[0, 0]), float(PIVOT[0, 1])
    return np.array([c, -s, px - (c * px - s * py) + x, s, c, py - (s * px + c * py) + y], dtype=np.float32)


def scene():
    """(scene lines (4, 12) float32, templates, the true record, the perturbed records, their planted poses (e, i, j))."""
    tmpl = polygon_lines(PART).astype(np.float32)
    true = R.records([0], [0.0], [pose_matrix(*TRUE_POSE)])
    lines = R.posed([tmpl], true[0]).astype(np.float32)
    recs, planted = [], []
    a0, x0, y0 = TRUE_POSE
    c, s = np.cos(a0), np.sin(a0)
    for da in ANGLES:
        for dx in SHIFTS_X:
            for dy in SHIFTS_Y:
                recs.append(pose_matrix(a0 + da, x0 + dx, y0 + dy))
                # the way back: the delta -da about the pivot (run position HALF_STEPS - da / STEP), then the shift (-dx, -dy)
                planted.append((HALF_STEPS - int(round(da / STEP)), -dx, -dy))
    # the unperturbed record goes first: the refined records tie on the score, and detect_matches then keeps the first
    mid = planted.index((HALF_STEPS, 0, 0))
    order = [mid] + [q for q in range(len(recs)) if q != mid]
    recs = R.records([0] * len(recs), np.zeros(len(recs)), [recs[q] for q in order])
    return lines, [tmpl], true, recs, np.array([planted[q] for q in order], dtype=np.int32)
