"""The definitions of include/fdcm.h, "line segments from images", in numpy: both orientation partitions of a label image,
their 8-connected components (scipy.ndimage.label), the votes, the kept components and their exact fit (Python ints for the
sums and their products, float() / np.float32 for the handful of float64 operations).  A referee: the library never imports
it."""
import numpy as np
from scipy import ndimage

EIGHT = np.ones((3, 3), dtype=bool)
MAX_PIXELS = 65535


def check_params(m, bucket, min_pixels, min_length):
    if not (1 <= m <= 255):
        raise ValueError("1 <= m <= 255")
    if not (1 <= bucket <= m):
        raise ValueError("bucket must be in [1, m]")
    if not (2 <= min_pixels <= MAX_PIXELS):
        raise ValueError("min_pixels must be in [2, 65535]")
    if not (1 <= min_length <= 4096):
        raise ValueError("min_length must be in [1, 4096]")


def buckets(labels, m, bucket):
    """(edge mask, bucket in partition A, bucket in partition B) per pixel, int64 (the buckets are -1 off the edges)."""
    lab = np.asarray(labels).astype(np.int64)
    edge = lab < m
    w, h = bucket, bucket // 2
    a = np.where(edge, lab // w, -1)
    b = np.where(edge, ((lab + h) % m) // w, -1)
    return edge, a, b


def components(bucket_image):
    """(component index per pixel, -1 where the bucket is -1; count): maximal 8-connected sets of equal bucket."""
    comp = np.full(bucket_image.shape, -1, dtype=np.int64)
    n = 0
    for b in np.unique(bucket_image[bucket_image >= 0]):
        lab, k = ndimage.label(bucket_image == b, structure=EIGHT)
        comp[lab > 0] = lab[lab > 0] - 1 + n
        n += k
    return comp, n


def fit(xs, ys):
    """(segment as 4 float32, length) of the pixels (xs, ys) by the definition's fit; at least two distinct pixels."""
    n = len(xs)
    xs, ys = [int(v) for v in xs], [int(v) for v in ys]
    Sx, Sy = sum(xs), sum(ys)
    Sxx, Syy, Sxy = sum(x * x for x in xs), sum(y * y for y in ys), sum(x * y for x, y in zip(xs, ys))
    Dxx, Dyy, Dxy = n * Sxx - Sx * Sx, n * Syy - Sy * Sy, n * Sxy - Sx * Sy
    assert max(abs(Dxx), abs(Dyy), abs(Dxy)) < 2 ** 56
    xb, yb = float(Sx) / float(n), float(Sy) / float(n)
    f32 = np.float32
    if Dxx >= Dyy:
        assert Dxx > 0
        x0, x1 = min(xs), max(xs)
        s = float(Dxy) / float(Dxx)
        Y = lambda x: yb + s * (float(x) - xb)
        return np.array([f32(x0), f32(Y(x0)), f32(x1), f32(Y(x1))], dtype=np.float32), x1 - x0 + 1
    assert Dyy > 0
    y0, y1 = min(ys), max(ys)
    s = float(Dxy) / float(Dyy)
    X = lambda y: xb + s * (float(y) - yb)
    return np.array([f32(X(y0)), f32(y0), f32(X(y1)), f32(y1)], dtype=np.float32), y1 - y0 + 1


def segments(labels, m, bucket, min_pixels, min_length):
    """((4, N) float32 in ascending 2 * root + partition, info).  info: `kept_b` kept components of partition B, `ties`
    components with 2 * votes == n (of at least two pixels), `keys` the kept components' 2 * root + partition, `pixels` per
    kept component its (ys, xs)."""
    check_params(m, bucket, min_pixels, min_length)
    labels = np.asarray(labels)
    assert labels.ndim == 2 and labels.dtype == np.uint8
    H, W = labels.shape
    edge, ba, bb = buckets(labels, m, bucket)
    info = dict(kept_b=0, ties=0, keys=[], pixels=[])
    if not edge.any():
        return np.zeros((4, 0), dtype=np.float32), info
    ys, xs = np.nonzero(edge)                       # row-major order: ascending y * W + x
    flat = ys * W + xs
    comp, size = [], []
    for img in (ba, bb):
        c, k = components(img)
        comp.append(c[ys, xs])
        size.append(np.bincount(comp[-1], minlength=k))
    votes_a = size[0][comp[0]] >= size[1][comp[1]]
    out = []
    for part in (0, 1):
        c, n = comp[part], size[part]
        votes = np.bincount(c[votes_a if part == 0 else ~votes_a], minlength=len(n))
        info["ties"] += int(((2 * votes == n) & (n >= 2)).sum())
        order = np.argsort(c, kind="stable")        # pixels grouped by component, row-major inside each
        first = np.concatenate([[0], np.cumsum(n)])
        for k in np.nonzero((2 * votes > n) & (n >= min_pixels) & (n <= MAX_PIXELS))[0]:
            idx = order[first[k]:first[k + 1]]
            seg, length = fit(xs[idx], ys[idx])
            if length >= min_length:
                out.append((2 * int(flat[idx[0]]) + part, seg, (ys[idx], xs[idx])))
    out.sort(key=lambda t: t[0])
    info["keys"] = [t[0] for t in out]
    info["pixels"] = [t[2] for t in out]
    info["kept_b"] = sum(k & 1 for k in info["keys"])
    if not out:
        return np.zeros((4, 0), dtype=np.float32), info
    return np.stack([t[1] for t in out], axis=1), info
