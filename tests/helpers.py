"""Shared test helpers: restatements of the reference's test utilities and the synthetic generators.

create_lines / make_rotation follow tests/test-utils/include/test-utils/utils.h:38-94 and
tests/python/test_matching.py:5-41 of the reference (inputs of its end-to-end tests).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

f32 = np.float32
U = 2.0 ** -24          # unit roundoff of float32


def make_rotation(angle):
    s, c = f32(np.sin(f32(angle))), f32(np.cos(f32(angle)))
    return np.array([[c, -s], [s, c]], dtype=np.float32)


def rotate_about(line, rot, pt):
    """core::rotate(line, rotation, rot_point), math.h:372-378."""
    line = np.asarray(line, dtype=np.float32).reshape(4, -1)
    pt = np.asarray(pt, dtype=np.float32)
    t = pt - rot @ pt
    pts = line.reshape(2, -1, order="F")
    out = (rot @ pts + t[:, None]).astype(np.float32)
    return out.reshape(4, -1, order="F")


def create_lines(n, length):
    """tests::createLines (utils.h:74-91): a fan of n lines from the origin, log-spaced angles in [2pi, 4pi]."""
    log_start = f32(np.log10(f32(2 * np.pi)))
    log_end = f32(np.log10(f32(4 * np.pi)))
    step = f32((log_end - log_start) / f32(n - 1))
    out = np.zeros((4, n), dtype=np.float32)
    for i in range(n):
        ang = f32(np.power(10.0, float(f32(log_start + f32(i) * step))))
        r = make_rotation(ang)
        out[2, i] = r[0, 0] * f32(length)
        out[3, i] = r[1, 0] * f32(length)
    return out


def apply_transform(lines, T):
    lines = np.asarray(lines, dtype=np.float32)
    T = np.asarray(T, dtype=np.float32)
    pts = lines.reshape(2, -1, order="F")
    return (T[:, :2] @ pts + T[:, 2:3]).astype(np.float32).reshape(4, -1, order="F")


# ---- the exact-owner statement of the L2 row pass (tests/test_exact_owner.py has the argument) ----
FMAX = np.float32(np.finfo(np.float32).max)


def exact_pass(f):
    """f: float32 vector (squares of integers or FLT_MAX) -> out[q] = base + (q - o)^2 with o the exact owner of q (the
    seeded column minimising f[u] + (q - u)^2, the smallest on a tie), base = f[o] for q <= o and out[o] for q > o."""
    n = len(f)
    cols = np.flatnonzero(f != FMAX)
    if len(cols) == 0:
        return f.copy()
    fi = f[cols].astype(np.int64)
    q = np.arange(n, dtype=np.int64)
    cost = fi[None, :] + (q[:, None] - cols[None, :]) ** 2       # [pixel][seeded column]
    owner = cols[np.argmin(cost, axis=1)]                          # argmin takes the first (smallest) column on a tie
    out = np.zeros(n, dtype=np.int64)
    fint = np.zeros(n, dtype=np.int64)
    fint[cols] = fi
    for p in range(n):
        o = owner[p]
        out[p] = (out[o] if o < p else fint[o]) + (p - o) ** 2
    assert out.max() < 2 ** 24 + 2 ** 23
    return out.astype(np.float32)


def exact_pass_rows(F):
    """exact_pass over every row of the (R, n) float32 array F at once (the same statement, vectorised)."""
    F = np.asarray(F, dtype=np.float32)
    R, n = F.shape
    out = F.copy()
    seeded = F != FMAX
    big = np.int64(1) << 60
    fi = np.where(seeded, F, 0).astype(np.int64)
    cost_f = np.where(seeded, fi, big)
    q = np.arange(n, dtype=np.int64)
    sq = (q[:, None] - q[None, :]) ** 2                            # [pixel][column]
    step = max(1, (1 << 23) // (n * n))
    for r0 in range(0, R, step):
        rows = slice(r0, min(R, r0 + step))
        owner = np.argmin(cost_f[rows, None, :] + sq[None, :, :], axis=2)   # first (smallest) column on a tie
        any_seed = seeded[rows].any(axis=1)
        base_fint = np.take_along_axis(fi[rows], owner, axis=1)
        d2 = (q[None, :] - owner) ** 2
        # out[p] = (out[o] if o < p else f[o]) + (p - o)^2: owners below p come first, so a fixed point is reached after
        # at most the length of the longest owner chain
        val = base_fint + d2
        below = owner < q[None, :]
        while True:
            nxt = np.where(below, np.take_along_axis(val, owner, axis=1), base_fint) + d2
            if np.array_equal(nxt, val):
                break
            val = nxt
        assert val[any_seed].max(initial=0) < 2 ** 24 + 2 ** 23
        out[rows] = np.where(any_seed[:, None], val.astype(np.float32), F[rows])
    return out


# ---- scenes the synthetic generator never builds ----
def _segments(rng, n, lo, hi, angles=None, min_len=0.0, max_len=None):
    """n float64 segments inside the box [lo, hi]^2 with the given angles (or uniform ones)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    out = np.zeros((4, n))
    span = float((hi - lo).max())
    max_len = span if max_len is None else max_len
    for i in range(n):
        while True:
            a = rng.uniform(0, np.pi) if angles is None else angles[i]
            L = rng.uniform(min_len, max_len)
            c = lo + rng.uniform(0, 1, size=2) * (hi - lo)
            d = 0.5 * L * np.array([np.cos(a), np.sin(a)])
            p1, p2 = c - d, c + d
            if (p1 >= lo).all() and (p1 <= hi).all() and (p2 >= lo).all() and (p2 <= hi).all():
                out[:, i] = (*p1, *p2)
                break
    return out


def edge_scenes():
    """[(name, (4, N) float32 scene, depth, coeff, padding)]: tiny maps, far-off coordinates, axis-parallel lines, lines
    of a single slice, depths 1, 2 and 180, coefficients 0 and 50, padding 1.0 and 3.7."""
    rng = np.random.default_rng(20261015)
    cases = [("point", np.array([[3.3], [7.6], [3.3], [7.6]]), 4, 5.0, 1.0)]
    # W = H = ceil(d + 1) for a bounding box of extent d and padding 1: the box's corners are drawn as two short lines
    for W, depth, coeff in [(2, 1, 5.0), (3, 2, 0.0), (4, 3, 50.0), (5, 4, 5.0), (7, 5, 5.0), (8, 6, 50.0),
                            (13, 7, 5.0), (16, 8, 0.0), (17, 12, 5.0), (24, 180, 5.0), (32, 30, 50.0)]:
        o = rng.uniform(-40, 40, size=2).round(2)
        d = W - 1 - rng.uniform(0.0, 0.9) if W > 2 else 1.0
        box = _segments(rng, max(1, W // 3), o, o + d)
        corners = np.array([[o[0], o[1], o[0] + min(0.5, d), o[1]], [o[0] + d, o[1] + d, o[0] + d, o[1] + d - min(0.5, d)]]).T
        cases.append((f"w{W}", np.concatenate([corners, box], axis=1), depth, coeff, 1.0))
    off = np.array([-5000.3, 12345.7])
    cases.append(("offset", _segments(rng, 24, off, off + 90.0, min_len=3.0, max_len=40.0), 12, 5.0, 1.0))
    cases.append(("offset-pad", _segments(rng, 16, off, off + 60.0, min_len=3.0, max_len=30.0), 7, 50.0, 3.7))
    ang = rng.integers(0, 2, size=30) * (np.pi / 2)
    cases.append(("axis", _segments(rng, 30, (0.5, 1.25), (120.5, 121.25), angles=ang, min_len=2.0, max_len=60.0), 8, 5.0, 1.0))
    cases.append(("axis-odd", _segments(rng, 20, (7.0, 3.0), (80.0, 76.0), angles=ang[:20], min_len=1.0, max_len=40.0), 5, 50.0, 3.7))
    # every line within a quarter of a slice of key 3 of depth 12 (-pi/2 + 3 pi/12 = -pi/4 = 3 pi/4 mod pi)
    ang1 = 0.75 * np.pi + rng.uniform(-0.25, 0.25, size=25) * np.pi / 12
    cases.append(("one-slice", _segments(rng, 25, (-20.0, -30.0), (100.0, 90.0), angles=ang1, min_len=5.0, max_len=50.0), 12, 50.0, 3.7))
    cases.append(("one-slice-vertical", _segments(rng, 12, (0.0, 0.0), (70.0, 70.0), angles=np.full(12, np.pi / 2), min_len=5.0), 2, 5.0, 1.0))
    cases.append(("depth180", _segments(rng, 40, (1.0, 2.0), (96.0, 97.0), min_len=4.0, max_len=40.0), 180, 50.0, 1.0))
    cases.append(("depth1", _segments(rng, 20, (0.0, 0.0), (60.0, 60.0), min_len=4.0, max_len=30.0), 1, 5.0, 3.7))
    return [(name, sc.astype(np.float32), depth, coeff, pad) for name, sc, depth, coeff, pad in cases]


EDGE_SCENES = {c[0]: c[1:] for c in edge_scenes()}


def definition_keys(m):
    """The m orientation keys k pi / m - pi / 2 in float64."""
    return np.arange(m) * np.pi / m - np.pi / 2


# ---- float64 re-scoring of a template on a volume (tests/test_definitions_dt3.py, tests/test_definitions_scoring.py) ----
def ulp32(x):
    return np.spacing(np.float32(np.max(np.abs(x)) if np.size(x) else 0.0)).astype(np.float64)



def nearest_bins(lines64, m, margin):
    """(4, N) float64 lines -> (bin, ambiguous) with bin the nearest of the m keys k pi / m - pi / 2 (circularly: an angle
    near pi/2 belongs to key 0) by a float64 arctan, ambiguous where the angle is within `margin` (per line) of the
    boundary between two keys or the line has no direction."""
    dx, dy = lines64[2] - lines64[0], lines64[3] - lines64[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.arctan(dy / dx)
    pos = (a + np.pi / 2) * m / np.pi                      # key units
    b = np.floor(pos + 0.5)
    frac = pos + 0.5 - b                                   # a boundary lies at frac 0 (and 1)
    amb = np.minimum(frac, 1 - frac) * np.pi / m < margin if m > 1 else np.zeros(len(pos), dtype=bool)
    amb |= ~np.isfinite(pos) | (np.hypot(dx, dy) < 1e-6)
    b = np.where(np.isfinite(b), b, 0).astype(np.int64) % m
    return b, amb


def rescore(vol, keys, lines64, W, H, err, aerr):
    """float64 score of a template whose (4, n) end points are already translated into the map: (score, bound, status)
    with status 'ok', 'outside' or 'ambiguous' (an end point within err of a pixel edge, or a line within 1e-5 rad plus
    the angle error of end points off by aerr of a bin boundary)."""
    m = len(keys)
    n = lines64.shape[1]
    if n == 0:
        return 0.0, 0.0, "ok"
    length = np.hypot(lines64[2] - lines64[0], lines64[3] - lines64[1])
    bins, amb = nearest_bins(lines64, m, 1e-5 + 2 * aerr / np.maximum(length, 1e-30))
    lim = np.array([W, H, W, H])[:, None]
    if ((lines64 <= -1 - err) | (lines64 >= lim + err)).any():     # truncates to a pixel outside the map
        return None, None, "outside"
    near = (np.abs(lines64 - np.round(lines64)) < err) & (np.round(lines64) != 0)  # cast<int>() truncates: 0 from both sides
    if near.any() or amb.any():
        return None, None, "ambiguous"
    ix = np.trunc(lines64).astype(np.int64)
    assert ((ix >= 0) & (ix < lim)).all()
    a = vol[bins, ix[0], ix[1]].astype(np.float64)
    c = vol[bins, ix[2], ix[3]].astype(np.float64)
    terms = np.abs(a - c)
    return float(terms.sum()), float(n * U * terms.sum()), "ok"
