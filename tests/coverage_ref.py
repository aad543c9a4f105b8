"""The definition of scene coverage (include/fdcm.h, "Scene coverage") in plain Python integers and numpy, the referee of
fdcm_scene_coverage.  Not collected: the tests import it.  Nothing here comes from the kernel.

The map gives its size (W, H), its scene translation T = (bx, by), whole pixels, and its keys.  Label pixel (px, py) is map
pixel (px + bx, py + by).  Line i of the pair (tmpl, a) -- rotation_ref.rotate_lines' float32 lines, or the lines as they are
without a table -- at the translation (x, y) has the end pixels trunc(fl(p + fl(T + t))) per coordinate, float32 sums: the two
map pixels whose integral values the line's cost subtracts.  The pose is admissible when every such sum lies in (-1, W) or
(-1, H).  The segment joins the two pixels, moved by -(bx, by); its bin is the closest orientation of the line
(oracle.closest_orientation on edge_ref.keys_of's keys, the host libm's atanf).  The window is nms_ref.footprints' box at the
margin, moved by (x, y) and cut to the image.  An edge pixel (label < m) of the window is explained when a line's bin is within
bin_tolerance of its label on the circle of m slices and its squared distance to the segment is <= radius^2 (near_segment)."""
import numpy as np

from nms_ref import footprints
from oracle import oracle as O
from rotation_ref import rotate_lines

f32 = np.float32


def near_segment(px, py, ax, ay, bx, by, radius):
    """Is (px, py) within `radius` of the segment A B?  Python integers: exact at any size."""
    px, py, ax, ay, bx, by, r2 = int(px), int(py), int(ax), int(ay), int(bx), int(by), int(radius) ** 2
    dx, dy, wx, wy = bx - ax, by - ay, px - ax, py - ay
    dot, len2 = wx * dx + wy * dy, dx * dx + dy * dy
    if dot <= 0:
        return wx * wx + wy * wy <= r2
    if dot >= len2:
        return (px - bx) ** 2 + (py - by) ** 2 <= r2
    cross = wx * dy - wy * dx
    return cross * cross <= r2 * len2


def bin_distance(l, b, m):
    """min(|l - b|, m - |l - b|) for integers or integer arrays."""
    d = np.abs(np.asarray(l, dtype=np.int64) - np.asarray(b, dtype=np.int64))
    return np.minimum(d, m - d)


def near_segment_many(px, py, ax, ay, bx, by, radius):
    """near_segment for int64 arrays that broadcast: pixels against one segment, or pixels (P, 1) against segments (N,).  Every
    coordinate is below 2^14 in magnitude here (asserted), so cross^2 and r^2 len2 stay below 2^62."""
    px, py, ax, ay, bx, by = (np.asarray(v, dtype=np.int64) for v in (px, py, ax, ay, bx, by))
    r2 = int(radius) ** 2
    assert all(v.size == 0 or np.abs(v).max() < 1 << 14 for v in (px, py, ax, ay, bx, by))
    dx, dy, wx, wy = bx - ax, by - ay, px - ax, py - ay
    dot, len2 = wx * dx + wy * dy, dx * dx + dy * dy
    cross = wx * dy - wy * dx
    return np.where(dot <= 0, wx * wx + wy * wy <= r2,
                    np.where(dot >= len2, (px - bx) ** 2 + (py - by) ** 2 <= r2, cross * cross <= r2 * len2))


def end_pixels(lines, T, W, H, x, y):
    """(admissible, (4, N) int64 map pixels ax, ay, bx, by) of the (4, N) float32 lines at the integer translation (x, y): the
    cost rule's float32 sums and truncation.  A NaN end point is not admissible; no lines are admissible anywhere."""
    lines = np.asarray(lines, dtype=np.float32).reshape(4, -1)
    offx, offy = f32(T[0]) + f32(int(x)), f32(T[1]) + f32(int(y))
    with np.errstate(invalid="ignore"):
        q = np.stack([lines[0] + offx, lines[1] + offy, lines[2] + offx, lines[3] + offy]).astype(np.float32)
        ok = bool(np.all((q[[0, 2]] > f32(-1)) & (q[[0, 2]] < f32(W))) and np.all((q[[1, 3]] > f32(-1)) & (q[[1, 3]] < f32(H))))
    if not ok:
        return False, np.zeros((4, 0), dtype=np.int64)
    return True, np.trunc(q).astype(np.int64)


def line_bins(lines, keys):
    lines = np.asarray(lines, dtype=np.float32).reshape(4, -1)
    return np.array([O.closest_orientation(keys, lines[:, i]) for i in range(lines.shape[1])], dtype=np.int64)


def frame(T, W, H, width, height):
    """(bx, by) of a map the section accepts."""
    bx, by = int(T[0]), int(T[1])
    assert bx >= 0 and by >= 0 and f32(bx) == f32(T[0]) and f32(by) == f32(T[1]), "the scene translation is not whole pixels"
    assert width + 2 * bx == W and height + 2 * by == H, "the map's size is not (width + 2 bx, height + 2 by)"
    return bx, by


def coverage(labels, keys, T, W, H, templates, poses, cs=None, pivots=None, radius=2, bin_tolerance=1, margin=None):
    """(counts (n, 2) int32, residual (height, width) uint8, masks) of the poses (n, 4): tmpl, a, x, y.  masks[q]: the (height,
    width) bool image of the pixels pose q explains (None for a pose that is not admissible)."""
    labels = np.asarray(labels)
    assert labels.ndim == 2 and labels.dtype == np.uint8
    height, width = labels.shape
    keys = np.asarray(keys, dtype=np.float32)
    m = len(keys)
    margin = radius if margin is None else margin
    assert 0 <= radius <= 32 and 0 <= bin_tolerance <= m // 2 and 0 <= margin <= 4096
    bx, by = frame(T, W, H, width, height)
    boxes = footprints(templates, cs, pivots, margin).astype(np.int64)
    csa = None if cs is None else np.asarray(cs, dtype=np.float32).reshape(-1, 2)
    poses = np.asarray(poses, dtype=np.int64).reshape(-1, 4)
    counts = np.zeros((len(poses), 2), dtype=np.int32)
    residual = labels.copy()
    masks, pairs = [], {}
    for q, (t, a, x, y) in enumerate(poses):
        if (t, a) not in pairs:
            tm = np.asarray(templates[t], dtype=np.float32).reshape(4, -1)
            if csa is not None:
                px, py = (0.0, 0.0) if pivots is None else pivots[t]
                tm = rotate_lines(tm, csa[a, 0], csa[a, 1], px, py)
            pairs[(t, a)] = (tm, line_bins(tm, keys))
        tm, bins = pairs[(t, a)]
        ok, ends = end_pixels(tm, T, W, H, x, y)
        if not ok:
            counts[q] = (-1, -1)
            masks.append(None)
            continue
        mask = np.zeros(labels.shape, dtype=bool)
        masks.append(mask)
        x0, y0, x1, y1 = boxes[t, a] + np.array([x, y, x, y])
        x0, y0, x1, y1 = max(0, x0), max(0, y0), min(width - 1, x1), min(height - 1, y1)
        if x0 > x1 or y0 > y1:
            continue
        ys, xs = np.nonzero(labels[y0:y1 + 1, x0:x1 + 1] < m)
        ys, xs = ys + y0, xs + x0
        labs = labels[ys, xs].astype(np.int64)
        hit = np.zeros(len(xs), dtype=bool)
        for i in range(0, tm.shape[1], 64):  # pixels x lines, 64 lines at a time
            e, b = ends[:, i:i + 64], bins[i:i + 64]
            near = near_segment_many(xs[:, None], ys[:, None], e[0] - bx, e[1] - by, e[2] - bx, e[3] - by, radius)
            hit |= ((bin_distance(labs[:, None], b, m) <= bin_tolerance) & near).any(axis=1)
        counts[q] = (len(xs), int(hit.sum()))
        mask[ys[hit], xs[hit]] = True
        residual[mask] = 255
    return counts, residual, masks
