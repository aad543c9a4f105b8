"""The end-to-end case of the image pyramid's tests: a synthetic 256 x 192 frame with three filled polygons of two shapes at
planted poses, the shapes' outlines as templates, and the coarse-to-fine chain in numpy over the CPU referees (pyramid_ref,
edge_ex_ref, the oracle's stages through edge_ref.reference_volume, window_detect_ref) -- the statement the device chain is
designed against.  Not collected: the tests import it."""
import numpy as np

import edge_ex_ref as X
import edge_ref
import nms_ref
import pyramid_ref as R
from oracle import oracle as O
from rotation_ref import rot_matrix, rotate_lines
from window_detect_ref import detect_windows_ref
from windows_ref import admissible_mask

f32 = np.float32
WIDTH, HEIGHT = 256, 192
BACKGROUND, VALUE = 60, 200
# two shapes without a symmetry, vertices in pixels about their own origin
SHAPES = [np.array([(-30, -20), (30, -20), (30, -4), (-8, -4), (-8, 20), (-30, 20)], dtype=np.float64),      # an L
          np.array([(-26, -14), (22, -22), (30, 16), (-6, 24)], dtype=np.float64)]                          # a scalene quadrilateral
# planted poses: (shape, fine angle index = degrees, translation x, y); none of the angles is on the coarse table
PLANTS = [(0, 37, 62, 58), (1, 152, 170, 60), (0, 281, 150, 136)]
FINE = np.deg2rad(np.arange(360.0))
COARSE = np.deg2rad(np.arange(36) * 10.0)
HALF_ANGLES = 10                    # a whole coarse step, in fine steps: a reduced frame's best coarse angle may be either neighbour
DEPTH, COEFF, BORDER = 180, 2.0, 2
EDGE = dict(threshold=80, low=40, smooth=1, min_pixels=8)
COARSE_OVERLAP, COARSE_MAX = 0.3, 12
# depth 180: the score sums a line along its bin's direction, so a bin of 1 degree is what resolves a fine step of 1 degree
# (at depth 12 the numpy chain's best poses sit on multiples of 15 degrees, at depth 60 within 2 degrees)
MAX_SCORE = 1.5                     # the numpy chain's planted poses score 0.29 to 0.66 at every level, its best junk job 3.6


def outline(poly):
    """(4, N) float32 lines of a closed polygon."""
    nxt = np.roll(poly, -1, axis=0)
    return np.ascontiguousarray(np.concatenate([poly, nxt], axis=1).T, dtype=np.float32)


def templates():
    return [outline(p) for p in SHAPES]


def posed_polygon(shape, degrees, tx, ty):
    """The shape's vertices under the pose in float64: rotated about the origin, then translated."""
    a = np.deg2rad(float(degrees))
    c, s = np.cos(a), np.sin(a)
    p = SHAPES[shape]
    return np.stack([c * p[:, 0] - s * p[:, 1] + tx, s * p[:, 0] + c * p[:, 1] + ty], axis=1)


def _inside(poly, px, py):
    """Even-odd rule at the points (px, py)."""
    inside = np.zeros(px.shape, dtype=bool)
    n = len(poly)
    for i in range(n):
        (x0, y0), (x1, y1) = poly[i], poly[(i + 1) % n]
        if y0 == y1:
            continue
        cross = ((y0 <= py) != (y1 <= py)) & (px < x0 + (py - y0) * (x1 - x0) / (y1 - y0))
        inside ^= cross
    return inside


def frame():
    """The (192, 256) uint8 frame: pixel (x, y) is the mean over a 4 x 4 sample grid of the unit square centred on (x, y)."""
    ss = 4
    yy, xx = np.mgrid[0:HEIGHT * ss, 0:WIDTH * ss]
    px, py = (xx + 0.5) / ss - 0.5, (yy + 0.5) / ss - 0.5
    img = np.full(px.shape, float(BACKGROUND))
    for shape, deg, tx, ty in PLANTS:
        img[_inside(posed_polygon(shape, deg, tx, ty), px, py)] = VALUE
    img = img.reshape(HEIGHT, ss, WIDTH, ss).mean(axis=(1, 3))
    out = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def recovered(records, fine_step=1):
    """Per planted pose whether some record has its template, a fine angle within one step and a translation within 1 px;
    and the number of records.  The templates rotate about the origin (pivot None), so a record's translation is its
    transform's last column."""
    cs = np.stack([np.cos(FINE), np.sin(FINE)], axis=1).astype(np.float32)
    found = []
    for shape, deg, tx, ty in PLANTS:
        ok = False
        for r in records:
            tr = r["transform"]
            a = np.nonzero((cs[:, 0] == tr[0]) & (cs[:, 1] == tr[3]))[0]
            d = min(abs(int(a[0]) - deg), 360 - abs(int(a[0]) - deg))
            ok |= int(r["tmpl_idx"]) == shape and d <= fine_step and abs(tr[2] - tx) <= 1 and abs(tr[5] - ty) <= 1
        found.append(bool(ok))
    return found, len(records)


# ---------------------------------------------------------------- the chain on the CPU
def cpu_map(image):
    """The oracle's feature map of an image: edge_ex_ref's labels, edge_ref's volume of them."""
    labels = X.edge_labels(image, DEPTH, EDGE["smooth"], EDGE["low"], EDGE["threshold"], EDGE["min_pixels"])
    keys, vol = edge_ref.reference_volume(labels, BORDER, DEPTH, COEFF, O.L2)
    return O.from_volume(keys, vol, (float(BORDER), float(BORDER)))


def score_planes(orc, tmpls, cs, master, stride=1, only=None):
    """Per template the (A, NY, NX) scores of M_a(template) on the stride-1 master grid, NaN where the translation is not
    admissible, off the stride's lattice, or -- with `only`, a bool (T, A, NY, NX) mask -- not asked for."""
    X0, Y0, NX, NY = master
    gx, gy = np.meshgrid(X0 + np.arange(NX), Y0 + np.arange(NY))
    pts = np.stack([gx, gy], axis=-1).reshape(-1, 2).astype(np.float32)
    lattice = ((gx % stride == 0) & (gy % stride == 0)).reshape(-1)
    out = []
    for t, tm in enumerate(tmpls):
        vol = np.full((len(cs), NY * NX), np.nan, dtype=np.float32)
        for a, (c, s) in enumerate(cs):
            lines = rotate_lines(tm, c, s)
            use = admissible_mask(lines, orc.translation, orc.W, orc.H, master).reshape(-1) & lattice
            if only is not None:
                use &= only[t, a].reshape(-1)
            if use.any():
                vol[a, use] = O.evaluate(orc, lines, pts[use])
        out.append(vol.reshape(len(cs), NY, NX))
    return out


def lengths(tmpls):
    return np.array([np.sqrt((tm[2] - tm[0]) ** 2 + (tm[3] - tm[1]) ** 2).sum(dtype=np.float32) for tm in tmpls], dtype=np.float32)


def greedy(cands, boxes, permille, max_det):
    """nms' greedy rule on (score, tmpl, a, tx, ty) candidates in ascending score."""
    left = sorted(cands)
    out = []
    while left and len(out) < max_det:
        d = left.pop(0)
        out.append(d)
        F = boxes[d[1], d[2]].astype(np.int64) + (d[3], d[4], d[3], d[4])
        keep = []
        for c in left:
            G = boxes[c[1], c[2]].astype(np.int64) + (c[3], c[4], c[3], c[4])
            inter = max(0, min(G[2], F[2]) - max(G[0], F[0]) + 1) * max(0, min(G[3], F[3]) - max(G[1], F[1]) + 1)
            union = (G[2] - G[0] + 1) * (G[3] - G[1] + 1) + (F[2] - F[0] + 1) * (F[3] - F[1] + 1) - inter
            if not 1000 * inter > permille * union:
                keep.append(c)
        left = keep
    return out


def coarse_seeds(orc, tmpls, stride, margin):
    """The coarse stage in numpy: per grid point the best (template, angle) by score / length, then the greedy rule.  Returns
    records in the map's own pixels."""
    from openfdcm_amd import _capi
    cs = np.stack([np.cos(COARSE), np.sin(COARSE)], axis=1).astype(np.float32)
    master = (-BORDER - 40, -BORDER - 40, orc.W + 80, orc.H + 80)
    planes = score_planes(orc, tmpls, cs, master, stride)
    den = np.maximum(lengths(tmpls), f32(1e-6))
    q = np.stack([planes[t] / den[t] for t in range(len(tmpls))])            # (T, A, NY, NX)
    T, A, NY, NX = q.shape
    flat = np.where(np.isnan(q), np.inf, q).reshape(T * A, NY * NX)
    pair = flat.argmin(axis=0)
    best = flat[pair, np.arange(NY * NX)]
    cands = [(float(best[g]), int(pair[g]) // A, int(pair[g]) % A, master[0] + g % NX, master[1] + g // NX)
             for g in np.nonzero(np.isfinite(best))[0]]
    boxes = nms_ref.footprints(tmpls, cs, None, margin=margin)
    picks = greedy(cands, boxes, int(round(1000 * COARSE_OVERLAP)), COARSE_MAX)
    rec = np.zeros(len(picks), dtype=_capi.MATCH_DTYPE)
    for l, (s, t, a, tx, ty) in enumerate(picks):
        M = rot_matrix(cs[a, 0], cs[a, 1])
        rec[l] = (t, s, [M[0, 0], M[0, 1], M[0, 2] + f32(tx), M[1, 0], M[1, 1], M[1, 2] + f32(ty)])
    return rec


def cpu_chain(level, coarse_stride=1):
    """The pyramid chain (coarse_stride 1 on level `level`) or, with level 0, the refined chain with a coarse stride, in numpy:
    (detections, jobs, seeds, every job's best score / length)."""
    import openfdcm_amd as fd
    img = frame()
    tmpls = templates()
    orc0 = cpu_map(img)
    orc_l = orc0 if level == 0 else cpu_map(R.level_image(img, level))
    small = [tm * f32(2.0 ** -level) for tm in tmpls]
    seeds = fd.lift_records(coarse_seeds(orc_l, small, coarse_stride, 0), level)
    half = max(2 ** level, coarse_stride)
    jobs = fd.pose_windows(seeds, COARSE, FINE, None, HALF_ANGLES, half, half, wrap=True)
    cs = np.stack([np.cos(FINE), np.sin(FINE)], axis=1).astype(np.float32)
    master = (-BORDER - 40, -BORDER - 40, orc0.W + 80, orc0.H + 80)
    only = np.zeros((len(tmpls), len(cs), master[3], master[2]), dtype=bool)
    for t, a0, na, x0, y0, nx, ny in jobs:
        for a in (a0 + np.arange(na)) % len(cs):
            only[t, a, y0 - master[1]:y0 - master[1] + ny, x0 - master[0]:x0 - master[0] + nx] = True
    vols = score_planes(orc0, tmpls, cs, master, 1, only)
    den = np.maximum(lengths(tmpls), f32(1e-6))
    boxes = nms_ref.footprints(tmpls, cs, None, margin=0)
    every = detect_windows_ref(vols, master, jobs, cs, None, 1, 1, den, boxes, np.inf, 4096, 1000)[0]
    dets = detect_windows_ref(vols, master, jobs, cs, None, 1, 1, den, boxes, MAX_SCORE, 1024, 300)[0]
    return dets, jobs, seeds, np.sort(every["score"])
