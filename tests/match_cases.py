"""The cases the tests of the calls on match lists share (include/fdcm.h, "Match lists").  Not collected: the tests import it.

Template sets with 0, 1, 3, 4, 8, 9, 33, 64, 65 and 130 lines (Eigen's packet boundaries and the kernel's rounds of 64 lanes),
four kinds of caps, an adopted 70 x 37 volume that holds a NaN and an infinity, and record lists that mix random rotations
inside the map with end points at -0.5, end points just outside, a NaN matrix entry, tmpl_idx out of range, negative and NaN
scores and duplicates."""
import numpy as np

import match_ref as R

f32 = np.float32
COUNTS = (0, 1, 3, 4, 8, 9, 33, 64, 65, 130)
SPAN = 24.0
LENGTHS = (1, 255, 256, 257, 700)
CAPS = ("none", "scalar", "zero", "mixed")


def template_set(seed=5, integer=False):
    """One template per line count of COUNTS, inside [0, SPAN]^2; integer: integer coordinates."""
    rng = np.random.default_rng(seed)
    out = []
    for n in COUNTS:
        c = rng.uniform(4, SPAN - 4, size=(2, n))
        a = rng.uniform(0, np.pi, size=n)
        h = rng.uniform(1.0, 4.0, size=n)
        d = np.stack([np.cos(a), np.sin(a)]) * h
        t = np.concatenate([c - d, c + d])
        out.append((np.rint(t) if integer else t).astype(np.float32))
    return out


def caps_of(templates, kind, seed=17):
    """None, or one float32 array of caps per template."""
    if kind == "none":
        return None
    lens = [R.line_lengths(t) for t in templates]
    if kind == "scalar":
        return [f32(1.5) * l for l in lens]
    if kind == "zero":
        return [np.zeros(len(l), dtype=np.float32) for l in lens]
    rng = np.random.default_rng(seed)
    return [np.where(rng.random(len(l)) < 0.4, np.inf, rng.uniform(0.0, 12.0, size=len(l))).astype(np.float32) for l in lens]


def adopted_volume():
    """(keys, vol [k][x][y], translation): 6 slices of 70 x 37 with a NaN and an infinity."""
    rng = np.random.default_rng(41)
    keys = np.unique(np.array([f32(f32(f32(i) * R.P.PIF) / f32(6)) - R.P.PI2F for i in range(6)], dtype=np.float32))
    vol = (rng.random((len(keys), 70, 37)) * 50).astype(np.float32)
    vol[2, 10:14, 5:9] = np.nan
    vol[4, 30:33, 20:24] = np.inf
    return keys, vol, np.array([3.5, -2.25], dtype=np.float32)


def record_list(seed, W, H, t, templates, n, base=0):
    """n records on a W x H map with scene translation t."""
    rng = np.random.default_rng(seed)
    T = len(templates)
    recs = np.zeros(n, dtype=R.MATCH_DTYPE)
    for j in range(n):
        ti = int(rng.integers(0, T))
        tm = np.asarray(templates[ti], dtype=np.float64).reshape(4, -1)
        kind = j % 16 if n > 16 else 0
        ang = 0.0 if kind in (10, 11) else rng.uniform(-np.pi, np.pi)
        c, s = np.cos(ang), np.sin(ang)
        xs = np.concatenate([c * tm[0] - s * tm[1], c * tm[2] - s * tm[3], [0.0]])
        ys = np.concatenate([s * tm[0] + c * tm[1], s * tm[2] + c * tm[3], [0.0]])
        lo = np.array([-xs.min(), -ys.min()]) + 0.25                       # the posed box inside [0, W - 1] x [0, H - 1]
        hi = np.array([W - 1.25 - xs.max(), H - 1.25 - ys.max()])
        p = lo + rng.random(2) * np.maximum(hi - lo, 0.0) - np.asarray(t, dtype=np.float64)
        score = rng.uniform(0.0, 40.0)
        if j % 3 == 0:
            score = np.round(score)                                        # ties
        M = np.array([c, -s, p[0], s, c, p[1]])
        if kind == 10:
            M[2] = -0.5 - xs.min() - float(t[0])                           # an end point at -0.5: inside (-1, W)
        elif kind == 11:
            if j % 32 == 11:
                M[2] = -1.0 - xs.min() - float(t[0])                       # an end point at -1: outside
            else:
                M[5] = H - ys.max() - float(t[1])                          # an end point at H: outside
        elif kind == 12:
            M[int(rng.integers(0, 6))] = np.nan if j % 32 == 12 else np.inf
        elif kind == 14:
            score = [-1.0, np.nan, -0.0, np.inf][(j // 16) % 4]
        idx = ti + base
        if kind == 13:                                                     # tmpl_idx out of range
            idx = [base - 1, base + T, base + T + 1000, -(1 << 31)][(j // 16) % 4]
        recs[j] = (np.int32(idx), f32(score), M.astype(np.float32))
        if kind == 15:
            recs[j] = recs[j - int(rng.integers(1, 15))]
    return recs


def canon(a):
    """Float arrays with every NaN as the one quiet NaN: what "byte for byte" compares (a NaN's payload is no result)."""
    a = np.array(a, dtype=np.float32, copy=True)
    a[np.isnan(a)] = np.float32(np.nan)
    return a


def same_floats(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and canon(a).tobytes() == canon(b).tobytes()


def same_records(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return (a.dtype == b.dtype == R.MATCH_DTYPE and a.shape == b.shape and np.array_equal(a["tmpl_idx"], b["tmpl_idx"])
            and same_floats(a["score"], b["score"]) and same_floats(a["transform"], b["transform"]))
