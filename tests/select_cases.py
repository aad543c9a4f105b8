"""The cases the tests of scene selection share (include/fdcm.h, "Scene selection"): the worlds of test_gpu_coverage.py without
a device, the parameter sets, the long list that crosses batches of rounds, the frame of the end-to-end test, and the section's
identities as checks on any (selected, counts, residual).  Not collected: the tests import it.  The referee's coverage of a list
is computed once per (world, list, radius) and shared; nothing here comes from the kernel."""
import functools

import numpy as np

import coverage_ref as CR
import edge_ref
import select_ref as SR
import test_gpu_coverage as G

WORLDS = ("96x80-b0-d30", "96x80-b5-d6", "70x37-b5-d30", "70x37-b5-d30-bytes")
PARAMS = [(c, s, p) for c in (0.0, 0.3) for s in (0.0, 0.5, 1.0) for p in (1, 3)]   # (min_coverage, min_new, min_pixels)
MAX_SELECTED = (1, 3, 4096)
RADII = (0, 2, 32)


class Case:
    """A label image, its frame, templates (with or without the table of angles) and a pose list."""

    def __init__(self, labels, depth, border, tmpls, poses, cs=None, pv=None):
        self.labels = np.ascontiguousarray(labels, dtype=np.uint8)
        self.labels.setflags(write=False)
        self.depth, self.border = depth, border
        self.keys = edge_ref.keys_of(depth)
        self.m = len(self.keys)
        self.height, self.width = self.labels.shape
        self.W, self.H = self.width + 2 * border, self.height + 2 * border
        self.tmpls, self.cs, self.pv = tmpls, cs, pv
        self.poses = np.ascontiguousarray(poses, dtype=np.int32).reshape(-1, 4)
        self._cov = {}

    def coverage(self, poses=None, labels=None, radius=2, bin_tolerance=1, margin=None):
        """coverage_ref.coverage; of the case's own list and labels, kept."""
        own = poses is None and labels is None
        key = (radius, bin_tolerance, margin)
        if own and key in self._cov:
            return self._cov[key]
        out = CR.coverage(self.labels if labels is None else labels, self.keys, (self.border, self.border), self.W, self.H, self.tmpls,
                          self.poses if poses is None else poses, self.cs, self.pv, radius=radius, bin_tolerance=bin_tolerance, margin=margin)
        if own:
            self._cov[key] = out
        return out

    def select(self, radius=2, bin_tolerance=1, margin=None, **kw):
        """The referee on the case's own list."""
        counts, _, masks = self.coverage(radius=radius, bin_tolerance=bin_tolerance, margin=margin)
        return SR.rule(self.labels, counts, masks, **kw)

    def windows(self, margin):
        """(n, 4) int64 x0, y0, x1, y1 of the poses' windows, cut to the image (x0 > x1 or y0 > y1: empty)."""
        from nms_ref import footprints
        boxes = footprints(self.tmpls, self.cs, self.pv, margin).astype(np.int64)
        p = self.poses.astype(np.int64)
        w = boxes[p[:, 0], p[:, 1]] + p[:, [2, 3, 2, 3]]
        return np.stack([np.maximum(0, w[:, 0]), np.maximum(0, w[:, 1]), np.minimum(self.width - 1, w[:, 2]),
                         np.minimum(self.height - 1, w[:, 3])], axis=1)

    def reversed(self):
        return Case(self.labels, self.depth, self.border, self.tmpls, self.poses[::-1], self.cs, self.pv)


@functools.lru_cache(maxsize=None)
def world(name, rot, reverse=False):
    """The world `name` of test_gpu_coverage.py with its list of about 60 poses: not admissible poses, empty windows, duplicates,
    an overlapping cluster, the 300-line template."""
    if reverse:
        return world(name, rot).reversed()
    import openfdcm_amd as fd
    width, height, border, depth, kind = G.WORLDS[name]
    labels = G.make_labels(width, height, depth, kind)
    m = len(edge_ref.keys_of(depth))
    tmpls = G.make_templates(width, height)
    rows = slice(1, int(tmpls[7][3, 0]) + 1)
    thin_x = int(np.argmax((labels[rows] < m).sum(axis=0)))
    poses = G.make_poses(width, height, border, 7 if rot else 1, thin_x)
    return Case(labels, depth, border, tmpls, poses, G.CS7 if rot else None, fd.template_pivots(tmpls) if rot else None)


@functools.lru_cache(maxsize=None)
def long_list():
    """270 poses of a one-line template on a 5-pixel lattice of the 96 x 80 world at depth 30: more than 128 are accepted at
    min_pixels = 1, so the rounds cross two batches of 64 and stop inside the third."""
    width, height, border, depth, kind = G.WORLDS["96x80-b0-d30"]
    labels = G.make_labels(width, height, depth, kind)
    tm = np.float32([[0.5], [0.5], [5.5], [3.5]])
    poses = [[0, 0, x, y] for y in range(0, 74, 5) for x in range(0, 88, 5)]
    return Case(labels, depth, border, [tm], poses)


LONG_KW = dict(radius=2, margin=2)   # bin_tolerance: m // 2

# ------------------------------------------------------------------------------------------------ end to end
BAR = np.float32([[0, 0], [23, 0], [23, 19], [0, 19]])   # a 23 x 19 bar, in its own frame
BAR_AT = (36, 60)


def outline(points):
    nxt = np.roll(points, -1, axis=0)
    return np.ascontiguousarray(np.concatenate([points, nxt], axis=1).T, dtype=np.float32)


def notch_frame():
    """160 x 120 at grey 60: the L-shaped part of test_gpu_coverage.py at 200, and a bar at 130 lying in its notch, two pixels
    from the part on both sides."""
    img = np.full((120, 160), 60, dtype=np.uint8)
    x0, y0 = G.PART_AT
    img[y0:y0 + 14, x0:x0 + 40] = 200
    img[y0 + 14:y0 + 34, x0:x0 + 16] = 200
    bx, by = BAR_AT
    img[by:by + 19, bx:bx + 23] = 130
    return img


def notch_candidates():
    (lx, ly), (bx, by) = G.PART_AT, BAR_AT
    return np.int32([[0, 0, lx, ly], [0, 0, lx + 1, ly], [1, 0, bx, by], [0, 0, lx, ly + 1], [1, 0, bx + 1, by + 1], [1, 0, bx - 1, by],
                     [0, 0, lx - 1, ly - 1]])


@functools.lru_cache(maxsize=None)
def notch():
    labels = edge_ref.edge_labels(notch_frame(), 30, 60)
    return Case(labels, 30, 0, [G.part_template(), outline(BAR)], notch_candidates())


# ------------------------------------------------------------------------------------------------ the identities
def check_identities(case, got, radius=2, bin_tolerance=1, margin=None, min_coverage=0.0, min_new=0.5, min_pixels=1, max_selected=1024,
                     coverage=None):
    """Identities 1, 2, 4 and 5 of the section on a result (selected, counts, residual) for the case's list; coverage: how to
    take scene coverage of a sub-list (poses -> (counts, residual)), the referee's by default."""
    sel, counts, residual = got
    labels = case.labels
    assert sel.dtype == np.int32 and counts.dtype == np.int32 and counts.shape == (len(sel), 3) and residual.dtype == np.uint8
    assert np.all(np.diff(sel) > 0) and len(sel) <= max_selected
    if coverage is None:
        def coverage(poses):
            return case.coverage(poses=poses, radius=radius, bin_tolerance=bin_tolerance, margin=margin)[:2]
    c, r = coverage(case.poses[sel])
    assert r.tobytes() == residual.tobytes() and np.array_equal(c, counts[:, :2])                      # 1
    assert int(counts[:, 2].sum()) == int((residual != labels).sum())                                  # 2
    assert len(sel) == 0 or counts[0, 2] == counts[0, 1]
    assert np.all(counts[:, 2] >= min_pixels) and np.all(1000 * counts[:, 2].astype(np.int64) >= SR.permille(min_new) * counts[:, 1])
    assert np.all(1000 * counts[:, 1].astype(np.int64) >= SR.permille(min_coverage) * counts[:, 0])
    chosen = [tuple(p) for p in case.poses[sel]]
    assert len(set(chosen)) == len(chosen)                                                             # 4
    if SR.permille(min_new) == 1000:                                                                   # 5
        assert np.array_equal(counts[:, 2], counts[:, 1])
        assert int(counts[:, 1].sum()) == int((residual != labels).sum())
