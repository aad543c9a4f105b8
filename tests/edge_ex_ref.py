"""The definitions of include/fdcm.h, "edges with smoothing, hysteresis and a minimum chain length", in numpy (int64
arithmetic): the smoothed image, the candidates and the strong ones, their 8-connected components by an explicit stack, and the
label image.  Sobel, the keys, the bins and the volume of a label image are edge_ref's.  Also the serpentine test image: one
long component whose only strong pixels are at one end."""
import numpy as np

import edge_ref
from oracle import oracle as O

NO_EDGE = edge_ref.NO_EDGE
KERNELS = {0: (np.array([1]), 0, 0), 1: (np.array([1, 2, 1]), 8, 4), 2: (np.array([1, 4, 6, 4, 1]), 128, 8)}
NEIGHBOURS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def check_params(smooth, low, high, min_pixels):
    if smooth not in (0, 1, 2):
        raise ValueError("smooth must be 0, 1 or 2")
    if not (edge_ref.THRESHOLD_MIN <= low <= high <= edge_ref.THRESHOLD_MAX):
        raise ValueError("1 <= low <= high <= 1442")
    if min_pixels < 1:
        raise ValueError("min_pixels must be >= 1")


def smooth_image(image, smooth):
    """S: the (H, W) uint8 image smoothed with w (x) w, I clamped to the image, rounded by the definition's shift."""
    img = np.asarray(image)
    assert img.ndim == 2 and img.dtype == np.uint8
    w, rnd, shift = KERNELS[smooth]
    if smooth == 0:
        return img.copy()
    H, W = img.shape
    p = np.pad(img.astype(np.int64), smooth, mode="edge")
    acc = np.zeros((H, W), dtype=np.int64)
    for j, wj in enumerate(w):
        for i, wi in enumerate(w):
            acc += wj * wi * p[j:j + H, i:i + W]
    out = (acc + rnd) >> shift
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def candidates(image, smooth, low, high):
    """(candidate mask, strong mask, gx, gy) of S.  edge_ref.sobel pads S itself with its edge pixels: the smoothed pixel at the
    clamped coordinate."""
    S = smooth_image(image, smooth)
    cand, gx, gy = edge_ref.edge_mask(S, low)
    m2 = gx * gx + gy * gy
    return cand, cand & (m2 >= int(high) ** 2), gx, gy


def components(mask):
    """(H, W) int64: -1 off the mask, else the index (0, 1, ...) of the pixel's 8-connected component; and the count."""
    H, W = mask.shape
    comp = np.full((H, W), -1, dtype=np.int64)
    n = 0
    for y0, x0 in zip(*np.nonzero(mask)):
        if comp[y0, x0] >= 0:
            continue
        comp[y0, x0] = n
        stack = [(y0, x0)]
        while stack:
            y, x = stack.pop()
            for dy, dx in NEIGHBOURS:
                v, u = y + dy, x + dx
                if 0 <= v < H and 0 <= u < W and mask[v, u] and comp[v, u] < 0:
                    comp[v, u] = n
                    stack.append((v, u))
        n += 1
    return comp, n


def edge_mask(image, smooth, low, high, min_pixels):
    """(edge mask, candidate mask, strong mask, gx, gy)."""
    check_params(smooth, low, high, min_pixels)
    cand, strong, gx, gy = candidates(image, smooth, low, high)
    comp, n = components(cand)
    size = np.bincount(comp[cand], minlength=n)
    has_strong = np.bincount(comp[strong], minlength=n) > 0
    keep = has_strong & (size >= min_pixels)
    edge = cand & keep[np.where(cand, comp, 0)] if n else np.zeros_like(cand)
    return edge, cand, strong, gx, gy


def labels_of(mask, gx, gy, depth):
    """edge_ref's labelling of the pixels of `mask`; one call of the oracle per distinct gradient."""
    keys = edge_ref.keys_of(depth)
    if len(keys) > 255:
        raise ValueError("more than 255 keys")
    out = np.full(mask.shape, NO_EDGE, dtype=np.uint8)
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return out
    pairs, inverse = np.unique(np.stack([gx[ys, xs], gy[ys, xs]], axis=1), axis=0, return_inverse=True)
    bins = np.array([O.closest_orientation(keys, (0.0, 0.0, float(-int(b)), float(int(a)))) for a, b in pairs], dtype=np.uint8)
    out[ys, xs] = bins[inverse.reshape(-1)]
    return out


def edge_labels(image, depth, smooth, low, high, min_pixels):
    """(H, W) uint8: the slice of every edge pixel, 255 elsewhere."""
    edge, _, _, gx, gy = edge_mask(image, smooth, low, high, min_pixels)
    return labels_of(edge, gx, gy, depth)


def farthest_steps(cand, strong):
    """Breadth-first over the candidates from all strong pixels at once: the largest number of 8-neighbour steps any reached
    candidate is from a strong pixel, and how many were reached."""
    H, W = cand.shape
    dist = np.full((H, W), -1, dtype=np.int64)
    frontier = list(zip(*np.nonzero(strong)))
    for y, x in frontier:
        dist[y, x] = 0
    d = 0
    while frontier:
        nxt = []
        for y, x in frontier:
            for dy, dx in NEIGHBOURS:
                v, u = y + dy, x + dx
                if 0 <= v < H and 0 <= u < W and cand[v, u] and dist[v, u] < 0:
                    dist[v, u] = d + 1
                    nxt.append((v, u))
        frontier = nxt
        d += 1
    return int(dist.max()), int((dist >= 0).sum())


def serpentine(width, height, ramp=True):
    """(height, width) uint8: stripes three rows thick every eight rows on a background of 70, value 80, joined alternately at
    the right and the left end into one band; the first 60 columns of the first stripe ramp down from 130 (the only strong
    gradients) unless ramp is False."""
    w, h = width, height
    img = np.full((h, w), 70, dtype=np.uint8)
    rows = list(range(6, h - 9, 8))
    for r in rows:
        img[r:r + 3, 5:w - 5] = 80
    for i in range(len(rows) - 1):
        c0 = w - 8 if i % 2 == 0 else 5
        img[rows[i]:rows[i + 1] + 3, c0:c0 + 3] = 80
    if ramp:
        for i in range(60):
            img[rows[0]:rows[0] + 3, 5 + i] = max(80, 130 - 2 * i)
    return img
