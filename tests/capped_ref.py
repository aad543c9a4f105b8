"""The numpy referee of the per-line caps (include/fdcm.h, "Per-line caps and line costs").  Not collected: the tests import it.

It never calls the capped path.  A one-line template's uncapped score is exactly the line's cost (the scalar tail, 0 + v),
so the cost map of every line comes from the uncapped score map of a set of one-line templates; a template's
admissibility comes from the NaNs of its own uncapped map.  The clamp (capped = cost > cap ? cap : cost, in float32: a NaN
cost stays NaN) and the sum in Eigen's order are stated here; the capped volumes then go to the referees that already
take volumes (peaks_ref, rotation_ref, windows_ref, detect_ref)."""
import numpy as np

f32 = np.float32


def clamp(cost, cap):
    """capped = cost > cap ? cap : cost, float32; a NaN cost stays NaN, cap +inf changes nothing."""
    cost, cap = np.asarray(cost, dtype=np.float32), np.asarray(cap, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(cost > cap, cap, cost).astype(np.float32)


def eigen_sum0(v):
    """VectorXf::sum() (Eigen 3.4.0, Packet4f) along axis 0 of a float32 array (n, ...): blocks of 8 in two packets,
    the trailing packet, predux (p[0] + p[2]) + (p[1] + p[3]), the scalar tail.  n = 0 gives +0."""
    v = np.asarray(v, dtype=np.float32)
    n = v.shape[0]
    if n == 0:
        return np.zeros(v.shape[1:], dtype=np.float32)
    a2, a1 = (n // 8) * 8, (n // 4) * 4
    with np.errstate(invalid="ignore", over="ignore"):
        if a1 == 0:
            res = v[0].copy()
            for i in range(1, n):
                res = res + v[i]
            return res
        p0 = v[0:4].copy()
        if a1 > 4:
            p1 = v[4:8].copy()
            for i in range(8, a2, 8):
                p0 = p0 + v[i:i + 4]
                p1 = p1 + v[i + 4:i + 8]
            p0 = p0 + p1
            if a1 > a2:
                p0 = p0 + v[a2:a2 + 4]
        res = (p0[0] + p0[2]) + (p0[1] + p0[3])
        for i in range(a1, n):
            res = res + v[i]
    return res.astype(np.float32)


def one_line_set(templates):
    """Every line of every template as a template of its own, in line order: ((4, 1) arrays, offsets of len + 1)."""
    out, offsets = [], [0]
    for t in templates:
        a = np.asarray(t, dtype=np.float32).reshape(4, -1)
        out += [a[:, i:i + 1].copy() for i in range(a.shape[1])]
        offsets.append(len(out))
    return out, np.asarray(offsets, dtype=np.int64)


def line_cost_maps(dev, templates, grid, cs=None, pivots=None):
    """(cost, offsets): cost[offsets[t] + i] is the uncapped cost map of line i of template t on the grid, (ny, nx) or with
    rotations cs (A, ny, nx), each rotation about the parent template's pivot.  From the uncapped score maps of one-line
    templates."""
    from openfdcm_amd.engine import DeviceTemplates
    lines, offsets = one_line_set(templates)
    if not lines:
        shape = (0, grid[3], grid[2]) if cs is None else (0, len(cs), grid[3], grid[2])
        return np.zeros(shape, dtype=np.float32), offsets
    ones = DeviceTemplates(lines)
    if cs is None:
        return dev.score_map(ones, grid), offsets
    pv = None if pivots is None else np.repeat(np.asarray(pivots, dtype=np.float32), np.diff(offsets), axis=0)
    return dev.rotation_score_map(ones, grid, cs, pv), offsets


def capped_volumes(cost, offsets, caps, uncapped):
    """The capped score volumes: per template the Eigen-order sum of its lines' clamped costs where its own uncapped map
    (uncapped[t], the same shape as one cost map) is not NaN, NaN elsewhere.  caps: one float32 array per template."""
    out = np.full(uncapped.shape, np.nan, dtype=np.float32)
    for t in range(len(offsets) - 1):
        c = np.asarray(caps[t], dtype=np.float32).reshape((-1,) + (1,) * (cost.ndim - 1))
        s = eigen_sum0(clamp(cost[offsets[t]:offsets[t + 1]], c)) if offsets[t + 1] > offsets[t] else np.zeros(uncapped.shape[1:], f32)
        adm = ~np.isnan(uncapped[t])
        out[t][adm] = s[adm]
    return out
