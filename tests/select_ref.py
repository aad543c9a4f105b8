"""The rule of scene selection (include/fdcm.h, "Scene selection") in plain Python, the referee of fdcm_scene_select.  Not
collected: the tests import it.  It stands on coverage_ref.coverage's counts and masks; nothing here comes from the kernel.

Pose q is a candidate when it is admissible, explained_q >= min_pixels and 1000 explained_q >= min_coverage_permille edges_q.
In list order, with C the claimed pixels: new_q = |E_q \\ C|; q is accepted when new_q >= min_pixels and
1000 new_q >= min_new_permille explained_q, and then C = C u E_q; the walk stops at max_selected accepted poses."""
import numpy as np

import coverage_ref as CR


def permille(v):
    return int(round(1000 * v))


def rule(labels, counts, masks, min_coverage=0.0, min_new=0.5, min_pixels=1, max_selected=1024):
    """The rule on coverage_ref.coverage's (counts, masks) of the list: (selected (k,) int32, counts (k, 3) int32 -- edges,
    explained, new --, residual (height, width) uint8)."""
    labels = np.asarray(labels)
    cov, share, min_pixels = permille(min_coverage), permille(min_new), int(min_pixels)
    assert 0 <= cov <= 1000 and 0 <= share <= 1000 and 1 <= min_pixels <= 1 << 24 and 1 <= max_selected <= 4096
    claimed = np.zeros(labels.shape, dtype=bool)
    selected, rows = [], []
    for q, mask in enumerate(masks):
        if len(selected) == max_selected:
            break
        edges, explained = int(counts[q][0]), int(counts[q][1])
        if mask is None or explained < min_pixels or 1000 * explained < cov * edges:
            continue
        new = int((mask & ~claimed).sum())
        if new >= min_pixels and 1000 * new >= share * explained:
            claimed |= mask
            selected.append(q)
            rows.append((edges, explained, new))
    residual = np.where(claimed, 255, labels).astype(np.uint8)
    return np.asarray(selected, dtype=np.int32), np.asarray(rows, dtype=np.int32).reshape(-1, 3), residual


def select(labels, keys, T, W, H, templates, poses, cs=None, pivots=None, radius=2, bin_tolerance=1, margin=None, **kw):
    counts, _, masks = CR.coverage(labels, keys, T, W, H, templates, poses, cs, pivots, radius, bin_tolerance, margin)
    return rule(labels, counts, masks, **kw)
