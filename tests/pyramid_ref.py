"""The definitions of include/fdcm.h, "image pyramid", in numpy: the level images from edge_ex_ref's smoothing sampled at the even
coordinates, the size recurrence, and the float32 rule by which a rotation search writes a record's transform (what lifting a
level's record relies on)."""
import numpy as np

import edge_ex_ref as X

MAX_LEVEL = 12


def level_size(width, height, level):
    """(W_l, H_l): W_(l+1) = (W_l + 1) >> 1."""
    for _ in range(level):
        width, height = (width + 1) >> 1, (height + 1) >> 1
    return width, height


def down(image):
    """P_(l+1) of P_l: S2(P_l) at (2x, 2y)."""
    return np.ascontiguousarray(X.smooth_image(image, 2)[::2, ::2])


def level_image(image, level):
    """P_level of the (H, W) uint8 image."""
    img = np.ascontiguousarray(image)
    assert img.ndim == 2 and img.dtype == np.uint8 and 0 <= level <= MAX_LEVEL
    for _ in range(level):
        img = down(img)
    assert img.shape[::-1] == level_size(image.shape[1], image.shape[0], level)
    return img


def record_transform(c, s, pivot, t):
    """The six float32 of a rotation search's record for the rotation (c, s) about `pivot` and the integer translation t: the
    library's M_a = [c, -s, m.x; s, c, m.y] with m = p - R p in float32, left to right, and the translation added in float32."""
    c, s = np.float32(c), np.float32(s)
    px, py = np.float32(pivot[0]), np.float32(pivot[1])
    ns = -s
    mx = px - (c * px + ns * py)
    my = py - (s * px + c * py)
    return np.array([c, ns, mx + np.float32(t[0]), s, c, my + np.float32(t[1])], dtype=np.float32)
