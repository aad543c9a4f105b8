"""The definitions of include/fdcm.h, "feature maps from images", in numpy: the label image of a uint8 image (int64
arithmetic; the bins through oracle.closest_orientation, so they are the host libm's bit for bit), and the volume of a label
image, assembled from the stage functions of the oracle that the line build's tests already rest on."""
import numpy as np

from helpers import FMAX
from oracle import oracle as O
from oracle import pyoracle as PO

NO_EDGE = 255
THRESHOLD_MIN, THRESHOLD_MAX = 1, 1442


def keys_of(depth):
    """The distinct float32 keys a line build of `depth` makes (dt3cpu.h:188-190)."""
    f32 = np.float32
    return np.unique(np.array([f32(f32(f32(i) * PO.PIF) / f32(depth)) - PO.PI2F for i in range(depth)], np.float32))


def sobel(image):
    """(gx, gy, m2) int64 arrays of an (H, W) uint8 image, replicate border."""
    img = np.asarray(image)
    assert img.ndim == 2 and img.dtype == np.uint8
    p = np.pad(img.astype(np.int64), 1, mode="edge")
    H, W = img.shape
    at = lambda dx, dy: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    gx = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    gy = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    return gx, gy, gx * gx + gy * gy


def edge_mask(image, threshold):
    """(edge mask, gx, gy) by the thinning rule."""
    if not (THRESHOLD_MIN <= int(threshold) <= THRESHOLD_MAX):
        raise ValueError(f"threshold must be in [{THRESHOLD_MIN}, {THRESHOLD_MAX}]")
    gx, gy, m2 = sobel(image)
    H, W = m2.shape
    a, b = np.abs(gx), np.abs(gy)
    diag = np.where((gx >= 0) == (gy >= 0), 1, -1)
    dx = np.where(29 * b < 12 * a, 1, np.where(29 * a < 12 * b, 0, 1))
    dy = np.where(29 * b < 12 * a, 0, np.where(29 * a < 12 * b, 1, diag))
    mp = np.pad(m2, 1)                                     # m2 = 0 outside the image
    yy, xx = np.mgrid[0:H, 0:W]
    before = mp[yy + 1 - dy, xx + 1 - dx]
    after = mp[yy + 1 + dy, xx + 1 + dx]
    return (m2 >= int(threshold) ** 2) & (m2 > before) & (m2 >= after), gx, gy


def edge_labels(image, depth, threshold):
    """(H, W) uint8: the slice of every edge pixel, 255 elsewhere."""
    keys = keys_of(depth)
    if len(keys) > 255:
        raise ValueError("more than 255 keys")
    edge, gx, gy = edge_mask(image, threshold)
    out = np.full(edge.shape, NO_EDGE, dtype=np.uint8)
    for y, x in zip(*np.nonzero(edge)):
        # the tangent (-gy, gx) as a line from the origin; the integer is negated first, so gy = 0 gives +0
        out[y, x] = O.closest_orientation(keys, (0.0, 0.0, float(-int(gy[y, x])), float(int(gx[y, x]))))
    return out


def reference_volume(labels, border, depth, coeff, distance, stop_after=3):
    """(keys, volume [k][x][y]) of a label image: per slice the 0 / FLT_MAX image and the reference's distance transform from
    there on, then its propagation and line integral, as oracle.build runs them."""
    labels = np.asarray(labels)
    keys = keys_of(depth)
    m = len(keys)
    h, w = labels.shape
    H, W = h + 2 * border, w + 2 * border
    vol = np.empty((m, W, H), dtype=np.float32)
    for k in range(m):
        img = np.full((H, W), FMAX, dtype=np.float32)
        img[border:border + h, border:border + w][labels == k] = 0
        if distance == O.L1:
            PO.column_pass_l1(img)
            t = np.ascontiguousarray(img.T)
            PO.column_pass_l1(t)
            img = np.ascontiguousarray(t.T)
        else:
            with np.errstate(all="ignore"):
                img = O.column_pass_l2(img)
                img = np.ascontiguousarray(O.column_pass_l2(np.ascontiguousarray(img.T)).T)
                if distance == O.L2:
                    img = np.sqrt(img)
        vol[k] = img.T
    if stop_after >= 2:
        vol = O.propagate(keys, vol, coeff)
    if stop_after >= 3:
        with np.errstate(over="ignore"):
            vol = np.stack([np.ascontiguousarray(O.line_integral(np.ascontiguousarray(vol[k].T), keys[k]).T) for k in range(m)])
    return keys, vol.astype(np.float32)


# ---- the test images: four rotated, filled, anti-aliased rectangles on a flat background plus Gaussian noise (sigma 6)
def synthetic_image(width, height, seed, n_rect=4, sigma=6.0):
    rng = np.random.default_rng(seed)
    ss = 4                                                   # supersampling per axis: the anti-aliasing
    yy, xx = np.mgrid[0:height * ss, 0:width * ss]
    px, py = (xx + 0.5) / ss, (yy + 0.5) / ss
    img = np.full((height * ss, width * ss), 70.0)
    small = min(width, height)
    for _ in range(n_rect):
        cx, cy = rng.uniform(0.2, 0.8) * width, rng.uniform(0.2, 0.8) * height
        hw, hh = rng.uniform(0.12, 0.3) * small, rng.uniform(0.08, 0.22) * small
        ang = rng.uniform(0, np.pi)
        c, s = np.cos(ang), np.sin(ang)
        u, v = (px - cx) * c + (py - cy) * s, -(px - cx) * s + (py - cy) * c
        img[(np.abs(u) <= hw) & (np.abs(v) <= hh)] = rng.uniform(120, 230)
    img = img.reshape(height, ss, width, ss).mean(axis=(1, 3))
    img += rng.normal(0.0, sigma, size=img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
